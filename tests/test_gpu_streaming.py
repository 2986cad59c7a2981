"""The streaming and reduction kernels of the training step -- BatchNorm statistics (stand-alone and finalized from the conv
epilogues' partials) / apply / backward, max-pool, the fused BatchNorm + ReLU + pool pair, bilinear x2, the 1x1 head (plain
and fused with BatchNorm + ReLU), the MSE + focal and SSIM losses, the anomaly score and Adam -- element by element against the float64 references of tests/_ref64.py,
through the C ABI, at the pixel counts where a loop bound goes wrong and at the shapes the benchmark runs.

Every bound is derived in _ref64.py and proved on the CPU in test_cpu_ref64.py; each kernel gets its own inputs (the
coefficients the backward reads are made by the test, not by the statistics kernel).  Each test prints one line
`REF64 <entry point> <dtype> <case> worst err/bound ...` so that a run shows how close a correct kernel comes
(profiles/ref64_streaming.txt holds the lines of one run)."""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

import _ref64 as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
SWEEP_PIXELS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 65, 127, 129, 255, 257, 511, 513, 4099, 16384 + 1, 512 * 32 - 1,
                512 * 32 + 1, 512 * 128 + 3]
SWEEP_C = [64, 128, 192, 1024]
EPS = 1e-5


@pytest.fixture(scope="module")
def hip():
    from tiaozhanbei_unet_amd import _lib, ops
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))      # host threads of the float64 references
    return _lib, ops


def dev():
    return torch.device("cuda:0")


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def gen(seed, shape, kind="normal"):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) if kind == "uniform" else torch.randn(shape, generator=g)


def nhwc(t, dtype):
    return t.to(dev()).to(dtype).contiguous(memory_format=torch.channels_last)


def cmp(dtype):
    return R.assert_bf16 if dtype == torch.bfloat16 else R.assert_fp32


def report(entry, dtype, case, **worst):
    print(f"\nREF64 {entry} {IDS[DTYPES.index(dtype)] if dtype in DTYPES else dtype} {case} " +
          " ".join(f"{k}={v:.3g}" for k, v in worst.items()), flush=True)


def coefficients(seed, c, mean_offset=0.3):
    """per-channel coefficients as one BatchNorm layer would hold them, made by the test: scale in [0.5, 1.5),
    beta = 0.3 randn, mean, istd in [0.5, 1.5); gamma = scale / istd and shift = beta - mean scale rounded to fp32"""
    scale = gen(seed, (c,), "uniform") + 0.5
    istd = gen(seed + 1, (c,), "uniform") + 0.5
    mean = gen(seed + 2, (c,)) * 0.2 + mean_offset
    gamma = scale / istd
    scale = gamma * istd
    shift = (gen(seed + 3, (c,)) * 0.3 - mean * scale)
    return gamma, mean, istd, scale, shift


def activations(seed, shape, offset=0.3, sigma=1.7):
    """1.7 randn + 0.3 (+ a per-channel offset vector) on the bf16 grid, NCHW logical order"""
    y = gen(seed, shape) * sigma
    off = offset if torch.is_tensor(offset) else torch.full((shape[1],), float(offset))
    return (y + off[None, :, None, None]).bfloat16().float()


# ------------------------------------------------------------------ the kernels, called on the test's own operands
def run_train_stats(L, ops, dtype, yd, gamma, beta, rm, rv, momentum):
    n, c, h, w = yd.shape
    pixels = n * h * w
    out = torch.empty(4, c, device=dev())
    need = L.lib().unet_bn_workspace(pixels, c)
    ws = torch.empty(need, dtype=torch.uint8, device=dev())
    rmd, rvd = (None, None) if rm is None else (rm.to(dev()).clone(), rv.to(dev()).clone())
    gd, bd = gamma.to(dev()), beta.to(dev())          # (held in names: a temporary could be freed before the kernel runs)
    L.check(L.lib().unet_bn_train_stats(ops._DT[dtype], p(yd), pixels, c, p(gd), p(bd), p(rmd),
                                        p(rvd), momentum, EPS, p(out[0]), p(out[1]), p(out[2]), p(out[3]), p(ws), need,
                                        st()), "bn stats")
    got = {"mean": out[0], "istd": out[1], "scale": out[2], "shift": out[3]}
    if rm is not None:
        got["running_mean"], got["running_var"] = rmd, rvd
    return got


def check_stats(got, ref, what):
    return {k: R.assert_fp32(got[k], ref[k], f"{what} {k}") for k in got}


def run_bn_bwd(L, ops, dtype, dad, yd, coef, frozen=False):
    gamma, mean, istd, scale, shift = (t.to(dev()) for t in coef)
    n, c, h, w = yd.shape
    pixels = n * h * w
    need = L.lib().unet_bn_workspace(pixels, c)
    ws = torch.empty(need, dtype=torch.uint8, device=dev())
    dy, dgb = torch.empty_like(yd), torch.empty(2, c, device=dev())
    f = L.lib().unet_bn_relu_bwd_frozen if frozen else L.lib().unet_bn_relu_bwd
    L.check(f(ops._DT[dtype], p(dad), p(yd), pixels, c, p(gamma), p(mean), p(istd), p(scale), p(shift), p(dgb[0]), p(dgb[1]),
              p(dy), p(ws), need, st()), "bn bwd")
    return dgb[0], dgb[1], dy


def check_bn_bwd(dtype, got, ref, what, sums_only=False):
    dg, db, dy = got
    w = {"dgamma": R.assert_fp32(dg, ref["dgamma"], what + " dgamma"), "dbeta": R.assert_fp32(db, ref["dbeta"], what + " dbeta")}
    if not sums_only:
        # No tie mask: the kernels take the ReLU mask from fmaf(y, scale, shift), whose sign is the sign of the exact value,
        # so nothing is left out of the dy comparison (0 of the 0.1 % a test may leave out).
        w["dy"] = cmp(dtype)(dy, ref["dy"], what + " dy")
    return w


def run_apply(L, ops, dtype, yd, scale, shift):
    n, c, h, w = yd.shape
    a = torch.empty_like(yd)
    sd, hd = scale.to(dev()), shift.to(dev())
    L.check(L.lib().unet_bn_relu_apply(ops._DT[dtype], p(yd), n * h * w, c, p(sd), p(hd), p(a), st()), "bn apply")
    return a


# ------------------------------------------------------------------ pixel-count sweep
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("c", SWEEP_C)
@pytest.mark.parametrize("pixels", SWEEP_PIXELS)
def test_bn_train_stats_pixel_sweep(hip, dtype, c, pixels):
    L, ops = hip
    shape = (1, c, 1, pixels)
    y = activations(1000 + pixels, shape, offset=(torch.arange(c) % 5).float() * 0.7)
    gamma, beta = gen(1, (c,), "uniform") + 0.5, gen(2, (c,)) * 0.3
    rm, rv = gen(3, (c,)) * 0.1, gen(4, (c,), "uniform") + 0.5
    worst = {}

    def merge(w):
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
    for momentum in (0.1, 1.0 / 3.0):          # (nn.BatchNorm2d(momentum=None) after three batches)
        got = run_train_stats(L, ops, dtype, nhwc(y, dtype), gamma, beta, rm, rv, momentum)
        ref = R.bn_train_stats(y, dtype, gamma, beta, rm, rv, momentum, EPS)
        merge(check_stats(got, ref, f"stats c={c} pixels={pixels}"))
    got = run_train_stats(L, ops, dtype, nhwc(y, dtype), gamma, beta, None, None, 0.1)      # running_* = NULL
    ref = R.bn_train_stats(y, dtype, gamma, beta, None, None, 0.1, EPS)
    merge(check_stats(got, ref, "stats without running"))
    if pixels == 1:
        e32 = float(torch.tensor(EPS, dtype=torch.float32))
        assert torch.equal(ref["var"][0], torch.zeros(c, dtype=torch.float64))
        assert float((got["istd"].cpu().double() - e32 ** -0.5).abs().max()) <= 2.0 ** -23 * e32 ** -0.5
        rvd = run_train_stats(L, ops, dtype, nhwc(y, dtype), gamma, beta, rm, rv, 0.1)["running_var"]
        assert bool(torch.isfinite(rvd).all())
    report("unet_bn_train_stats", dtype, f"c={c},pixels={pixels}", **worst)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("c", SWEEP_C)
@pytest.mark.parametrize("pixels", SWEEP_PIXELS)
def test_bn_relu_apply_and_bwd_pixel_sweep(hip, dtype, c, pixels):
    L, ops = hip
    shape = (1, c, 1, pixels)
    coef = coefficients(2000 + c, c)
    y, da = activations(2000 + pixels, shape), activations(3000 + pixels, shape, offset=0.5, sigma=1.0)
    yd, dad = nhwc(y, dtype), nhwc(da, dtype)
    worst = {"a": cmp(dtype)(run_apply(L, ops, dtype, yd, coef[3], coef[4]), R.bn_relu_apply(y, dtype, coef[3], coef[4]),
                             f"apply c={c} pixels={pixels}")}
    for frozen in (False, True):
        ref = R.bn_relu_bwd(da, y, dtype, *coef, frozen=frozen)
        w = check_bn_bwd(dtype, run_bn_bwd(L, ops, dtype, dad, yd, coef, frozen), ref, f"bwd c={c} pixels={pixels} frozen={frozen}")
        worst.update({k + ("_frozen" if frozen else ""): v for k, v in w.items()})
    report("unet_bn_relu_apply/_bwd/_bwd_frozen", dtype, f"c={c},pixels={pixels}", **worst)


# ------------------------------------------------------------------ fused BatchNorm + ReLU + pool, premasked backward
def run_pool_pair(L, ops, dtype, y, dpooled, da_old, coef, what):
    """unet_bn_relu_pool_fwd, unet_bn_relu_pool_bwd (da_old NULL and given), unet_bn_bwd_premasked on its partials"""
    gamma, mean, istd, scale, shift = coef
    n, c, h, w = y.shape
    dt = ops._DT[dtype]
    yd, gd = nhwc(y, dtype), nhwc(dpooled, dtype)
    cd = [t.to(dev()) for t in coef]
    a, pooled = torch.empty_like(yd), torch.empty_like(gd)
    L.check(L.lib().unet_bn_relu_pool_fwd(dt, p(yd), n, h, w, c, p(cd[3]), p(cd[4]), p(a), p(pooled), st()), "pool fwd")
    worst = {"a": cmp(dtype)(a, R.bn_relu_apply(y, dtype, scale, shift), what + " a")}
    assert torch.equal(pooled, F.max_pool2d(a.float(), 2).to(dtype)), what + ": pooled is not the 2x2 max of the stored a"
    assert torch.equal(a, run_apply(L, ops, dtype, yd, scale, shift)), what + ": fused a differs from unet_bn_relu_apply"
    for old in (None, da_old):
        tag = what + (" da_old=NULL" if old is None else " da_old")
        od = None if old is None else nhwc(old, dtype)
        dz = torch.empty_like(yd)
        part = torch.empty((L.lib().unet_bn_relu_pool_max_parts(), 2, c), dtype=torch.float32, device=dev())
        nparts = C.c_int32(0)
        L.check(L.lib().unet_bn_relu_pool_bwd(dt, p(yd), p(gd), p(od), n, h, w, c, p(cd[3]), p(cd[4]), p(cd[1]), p(dz), p(part),
                                              C.byref(nparts), st()), "pool bwd")
        ref = R.bn_relu_pool_bwd(y, dpooled, old, dtype, scale, shift, mean)
        k = "" if old is None else "_old"
        worst["dz" + k] = cmp(dtype)(dz, ref["dz"], tag + " dz")
        assert torch.equal(dz.double().cpu(), ref["dz_stored"]), tag + ": dz is not the routed gradient rounded once"
        sums = part[:nparts.value].double().sum(0).cpu()           # the ordered fp64 finalize of the partials, on the host
        worst["sum" + k] = R.assert_fp32(sums[0], ref["sum"], tag + " sum dz")
        worst["sum_c" + k] = R.assert_fp32(sums[1], ref["sum_c"], tag + " sum dz (y - mean)")
        dy, dgb = torch.empty_like(yd), torch.empty(2, c, device=dev())
        ws = torch.empty(3 * c, device=dev())
        L.check(L.lib().unet_bn_bwd_premasked(dt, p(dz), p(yd), n * h * w, c, p(cd[0]), p(cd[1]), p(cd[2]), p(part), nparts.value,
                                              p(dgb[0]), p(dgb[1]), p(dy), p(ws), 3 * c * 4, st()), "premasked")
        pm = R.bn_bwd_premasked(ref["dz_stored"], R.rd(y, dtype), torch.float64, gamma, mean, istd)
        worst["dgamma" + k] = R.assert_fp32(dgb[0], pm["dgamma"], tag + " dgamma")
        worst["dbeta" + k] = R.assert_fp32(dgb[1], pm["dbeta"], tag + " dbeta")
        worst["dy" + k] = cmp(dtype)(dy, pm["dy"], tag + " dy")
    return worst


POOL_FRAMES = [(1, 2, 2), (1, 3, 3), (1, 2, 17), (2, 5, 7), (1, 33, 31), (1, 64, 65), (3, 127, 9), (1, 256, 257)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("c", SWEEP_C)
@pytest.mark.parametrize("frame", POOL_FRAMES, ids=str)
def test_bn_relu_pool_and_premasked_frame_sweep(hip, dtype, c, frame):
    """even and odd frames (the floor-dropped row and column get no pooled gradient: dz = da_old there, 0 without one)"""
    L, ops = hip
    n, h, w = frame
    if not L.lib().unet_bn_relu_pool_supported(ops._DT[dtype], c):
        z = torch.zeros(1, c, 2, 2, device=dev(), dtype=dtype)
        rc = L.lib().unet_bn_relu_pool_fwd(ops._DT[dtype], p(z), 1, 2, 2, c, p(z), p(z), p(z), p(z), st())
        assert rc == -2 and b"unet_bn_relu_pool_fwd" in L.lib().unet_last_error()       # refused, and says so
        pytest.skip(f"unet_bn_relu_pool_* refuses c={c} (checked: status and message)")
    if c == 1024 and h * w > 5000:
        n, h, w = 1, h // 4 + 1, w // 4            # keep the 1024-channel frames small; still odd / even as listed
    coef = coefficients(4000 + c, c)
    y = activations(4000 + h * w, (n, c, h, w))
    dpooled = activations(4100 + h * w, (n, c, h // 2, w // 2), offset=0.5, sigma=1.0)
    da_old = activations(4200 + h * w, (n, c, h, w), offset=0.5, sigma=1.0)
    worst = run_pool_pair(L, ops, dtype, y, dpooled, da_old, coef, f"pool c={c} frame={frame}")
    report("unet_bn_relu_pool_fwd/_bwd + unet_bn_bwd_premasked", dtype, f"c={c},frame={n}x{h}x{w}", **worst)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pool_ties_zeros_and_negative_zeros(hip, dtype):
    """channel 0: every window a four-way tie (the gradient goes to the first pixel); channel 1: pre-activation exactly 0 and
    -0 (mask off, a = +0); channel 2: ties between a positive value and itself across the window's second row"""
    L, ops = hip
    n, c, h, w = 2, 64, 13, 10
    gamma, mean, istd, scale, shift = coefficients(5000, c)
    shift[1] = 0.0
    coef = (gamma, mean, istd, scale, shift)
    y = activations(5001, (n, c, h, w))
    y[:, 0] = 0.75
    y[:, 1, ::2] = 0.0
    y[:, 1, 1::2] = -0.0
    y[:, 2, 1::2] = y[:, 2, 0:h - 1:2]
    dpooled = activations(5002, (n, c, h // 2, w // 2), offset=0.5, sigma=1.0)
    da_old = activations(5003, (n, c, h, w), offset=0.5, sigma=1.0)
    worst = run_pool_pair(L, ops, dtype, y, dpooled, da_old, coef, "pool ties")
    # the same edges through the unfused kernels: bit for bit
    x = nhwc(y, dtype)
    xq = R.rd(y, dtype)
    out = torch.empty((n, c, h // 2, w // 2), dtype=dtype, device=dev(), memory_format=torch.channels_last)
    L.check(L.lib().unet_maxpool2_fwd(ops._DT[dtype], p(x), n, h, w, c, p(out), st()), "maxpool fwd")
    assert torch.equal(out.double().cpu(), R.maxpool2(xq))
    g, gpd = R.rd(dpooled, dtype), nhwc(dpooled, dtype)
    routed = R.maxpool2_route(xq, g)
    assert float(routed[:, 0, 1::2].abs().max()) == 0 and float(routed[:, 0, :, 1::2].abs().max()) == 0
    dx = torch.full_like(x, 7.0)
    L.check(L.lib().unet_maxpool2_bwd(ops._DT[dtype], p(x), p(gpd), n, h, w, c, p(dx), 0, st()), "maxpool bwd")
    assert torch.equal(dx.double().cpu(), routed), "maxpool bwd: first maximum / zero on the floor-dropped row"
    base = R.rd(da_old, dtype)
    dx = nhwc(da_old, dtype).clone(memory_format=torch.channels_last)
    L.check(L.lib().unet_maxpool2_bwd(ops._DT[dtype], p(x), p(gpd), n, h, w, c, p(dx), 1, st()), "maxpool acc")
    worst["acc"] = cmp(dtype)(dx, (base + routed, base.abs() + routed.abs()), "maxpool bwd accumulate")
    # ReLU edges through unet_bn_relu_bwd: z = +0 and -0 are off
    ref = R.bn_relu_bwd(da_old, y, dtype, *coef)
    assert not bool(ref["on"][:, 1].any())
    worst.update(check_bn_bwd(dtype, run_bn_bwd(L, ops, dtype, nhwc(da_old, dtype), x, coef), ref, "bwd at exact zeros"))
    report("pool ties / ReLU zeros", dtype, "2x64x13x10", **worst)


# ------------------------------------------------------------------ real shapes
REAL_LEVELS = [(64, 256, 256), (128, 128, 128), (256, 64, 64), (512, 32, 32), (1024, 16, 16)]
N_ELEMENTWISE = 2          # element-wise outputs: batch 2 (float64 references of about 0.5 GiB per tensor at the largest)


def offsets(c, seed):
    """per-channel offsets of 1 to 3 sigma, either sign: what makes a missing row group visible (see _ref64)"""
    o = (gen(seed, (c,), "uniform") * 2 + 1) * torch.where(gen(seed + 1, (c,)) > 0, 1.0, -1.0)
    assert float(o.abs().min()) >= R.MIN_STREAM_OFFSET
    return o


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bn_sums_at_the_benchmark_reduction_length(hip, dtype):
    """(32, 64, 256, 256): statistics and backward sums over 2 097 152 pixels per channel"""
    L, ops = hip
    shape = (32, 64, 256, 256)
    assert shape[0] * shape[2] * shape[3] <= R.MAX_STREAM_PIXELS
    c = shape[1]
    y = activations(6000, shape, offset=offsets(c, 6001) * 1.7)
    gamma, beta = gen(1, (c,), "uniform") + 0.5, gen(2, (c,)) * 0.3
    rm, rv = gen(3, (c,)) * 0.1, gen(4, (c,), "uniform") + 0.5
    yd = nhwc(y, dtype)
    ref = R.bn_train_stats(y, dtype, gamma, beta, rm, rv, 0.1, EPS)
    worst = check_stats(run_train_stats(L, ops, dtype, yd, gamma, beta, rm, rv, 0.1), ref, "stats at 2097152 pixels")
    report("unet_bn_train_stats", dtype, "32x64x256x256", **worst)
    del ref
    # backward sums: coefficients that belong to this y (mean / istd of the data, rounded to fp32), gradient with an offset
    mean, istd = y.double().mean((0, 2, 3)).float(), y.double().var((0, 2, 3), unbiased=False).add(EPS).rsqrt().float()
    scale = gamma * istd
    coef = (gamma, mean, istd, scale, beta - mean * scale)
    da = activations(6002, shape, offset=offsets(c, 6003), sigma=1.0)
    got = run_bn_bwd(L, ops, dtype, nhwc(da, dtype), yd, coef)
    yq, daq = R.rd(y, dtype), R.rd(da, dtype)
    del y, da
    daq *= (yq * R._c(scale) + R._c(coef[4])) > 0
    db = (daq.sum((0, 2, 3)), daq.abs().sum((0, 2, 3)))
    yq -= R._c(mean)
    yq *= R._c(istd)
    daq *= yq
    dg = (daq.sum((0, 2, 3)), daq.abs().sum((0, 2, 3)))
    worst = {"dgamma": R.assert_fp32(got[0], dg, "dgamma at 2097152 pixels"), "dbeta": R.assert_fp32(got[1], db, "dbeta at 2097152 pixels")}
    report("unet_bn_relu_bwd (sums)", dtype, "32x64x256x256", **worst)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(N_ELEMENTWISE,) + s for s in REAL_LEVELS] + [(2, 64, 1408, 512), (2, 1024, 88, 32)], ids=str)
def test_bn_at_real_shapes(hip, dtype, shape):
    L, ops = hip
    c = shape[1]
    y = activations(7000 + c, shape, offset=offsets(c, 7001) * 1.7)
    gamma, beta = gen(1, (c,), "uniform") + 0.5, gen(2, (c,)) * 0.3
    rm, rv = gen(3, (c,)) * 0.1, gen(4, (c,), "uniform") + 0.5
    yd = nhwc(y, dtype)
    ref = R.bn_train_stats(y, dtype, gamma, beta, rm, rv, 0.1, EPS)
    worst = check_stats(run_train_stats(L, ops, dtype, yd, gamma, beta, rm, rv, 0.1), ref, f"stats {shape}")
    mean, istd = ref["mean"][0].float(), ref["istd"][0].float()
    scale = gamma * istd
    coef = (gamma, mean, istd, scale, beta - mean * scale)
    worst["a"] = cmp(dtype)(run_apply(L, ops, dtype, yd, coef[3], coef[4]), R.bn_relu_apply(y, dtype, coef[3], coef[4]), f"apply {shape}")
    da = activations(7002 + c, shape, offset=offsets(c, 7003), sigma=1.0)
    ref = R.bn_relu_bwd(da, y, dtype, *coef)
    worst.update(check_bn_bwd(dtype, run_bn_bwd(L, ops, dtype, nhwc(da, dtype), yd, coef), ref, f"bwd {shape}"))
    report("unet_bn_train_stats/_relu_apply/_relu_bwd", dtype, "x".join(map(str, shape)), **worst)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(2, 64, 256, 256), (2, 512, 32, 32), (1, 64, 1408, 512)], ids=str)
def test_pool_pair_at_real_shapes(hip, dtype, shape):
    """(1, 64, 1408, 512) has 180 224 windows x 8 (bf16) / 16 (fp32) channel groups: the backward's grid is capped at
    unet_bn_relu_pool_max_parts() = 2048 blocks, every thread walks several windows, and unet_bn_bwd_premasked gets 2048
    partials (its 64-lane finalize; the small frames of the sweep give fewer than 128 and take the 16-lane one)."""
    L, ops = hip
    n, c, h, w = shape
    y = activations(8000 + c, shape, offset=offsets(c, 8001) * 1.7)
    mean = y.double().mean((0, 2, 3)).float()
    istd = y.double().var((0, 2, 3), unbiased=False).add(EPS).rsqrt().float()
    gamma, beta = gen(1, (c,), "uniform") + 0.5, gen(2, (c,)) * 0.3
    scale = gamma * istd
    coef = (gamma, mean, istd, scale, beta - mean * scale)
    dpooled = activations(8002, (n, c, h // 2, w // 2), offset=offsets(c, 8003), sigma=1.0)
    da_old = activations(8004, shape, offset=offsets(c, 8005), sigma=1.0)
    worst = run_pool_pair(L, ops, dtype, y, dpooled, da_old, coef, f"pool {shape}")
    report("unet_bn_relu_pool_fwd/_bwd + unet_bn_bwd_premasked", dtype, "x".join(map(str, shape)), **worst)


# ------------------------------------------------------------------ cancellation in var = E[y^2] - mean^2
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bn_statistics_of_channels_with_large_means(hip, dtype):
    """per-channel mean of 0, 1, 30 and 300 sigma, a constant channel and a channel that is zero but for one pixel, inputs on
    the bf16 grid: the derived bound widens with mean^2 / var, and the kernel has to stay inside it"""
    L, ops = hip
    shape = (4, 64, 128, 128)
    c = shape[1]
    sig = torch.tensor([0.0, 1.0, 30.0, 300.0]).repeat(c // 4)
    y = activations(9000, shape, offset=sig * 1.7)
    y[:, 4] = 2.75
    y[:, 5] = 0.0
    y[1, 5, 17, 3] = 1.5
    gamma, beta = gen(1, (c,), "uniform") + 0.5, gen(2, (c,)) * 0.3
    rm, rv = gen(3, (c,)) * 0.1, gen(4, (c,), "uniform") + 0.5
    got = run_train_stats(L, ops, dtype, nhwc(y, dtype), gamma, beta, rm, rv, 0.1)
    ref = R.bn_train_stats(y, dtype, gamma, beta, rm, rv, 0.1, EPS)
    seen = (got["istd"].double().cpu() - ref["istd"][0]).abs() / ref["istd"][0]
    rows = [("0 sigma", 0), ("1 sigma", 1), ("30 sigma", 2), ("300 sigma", 3), ("constant 2.75", 4), ("one pixel", 5)]
    for name, ch in rows:
        pick = [ch] if ch >= 4 else [k for k in range(ch, c, 4) if k not in (4, 5)]
        print(f"\nREF64 istd {IDS[DTYPES.index(dtype)]} {name}: allowed rel {float(ref['istd_rel'][pick].min()):.3e} "
              f"observed rel {float(seen[pick].max()):.3e}", flush=True)
    worst = check_stats(got, ref, "stats with large means")
    report("unet_bn_train_stats", dtype, "cancellation 4x64x128x128", **worst)


# ------------------------------------------------------------------ eval coefficients
def test_bn_eval_coeffs(hip):
    L, ops = hip
    c = 192
    gamma, beta = gen(1, (c,), "uniform") + 0.5, gen(2, (c,)) * 0.3
    rm, rv = gen(3, (c,)) * 3, gen(4, (c,), "uniform") * 2
    rv[:3] = torch.tensor([0.0, 1e-12, 1e6])
    out = torch.empty(4, c, device=dev())
    gd, bd, rmd, rvd = (t.to(dev()) for t in (gamma, beta, rm, rv))
    L.check(L.lib().unet_bn_eval_coeffs4(c, p(gd), p(bd), p(rmd), p(rvd), EPS, p(out[0]),
                                         p(out[1]), p(out[2]), p(out[3]), st()), "eval4")
    ref = R.bn_eval_coeffs(gamma, beta, rm, rv, EPS)
    assert torch.equal(out[0].cpu(), rm)
    worst = {k: R.assert_fp32(out[i], ref[k], "eval " + k) for i, k in ((1, "istd"), (2, "scale"), (3, "shift"))}
    out2 = torch.empty(2, c, device=dev())
    L.check(L.lib().unet_bn_eval_coeffs(c, p(gd), p(bd), p(rmd), p(rvd), EPS, p(out2[0]),
                                        p(out2[1]), st()), "eval")
    assert torch.equal(out2, out[2:])
    report("unet_bn_eval_coeffs(4)", "fp32", "c=192", **worst)


# ------------------------------------------------------------------ max-pool and bilinear at real shapes, bilinear edges
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(2, 64, 256, 256), (2, 1024, 16, 16), (1, 64, 1407, 511)], ids=str)
def test_maxpool_bit_for_bit_at_real_shapes(hip, dtype, shape):
    L, ops = hip
    n, c, h, w = shape
    x = activations(10000 + c, shape).clamp_min(0)                   # post-ReLU: whole windows of zeros tie
    xd, xq = nhwc(x, dtype), R.rd(x, dtype)
    g = activations(10001, (n, c, h // 2, w // 2), sigma=1.0)
    gpd = nhwc(g, dtype)
    out = torch.empty((n, c, h // 2, w // 2), dtype=dtype, device=dev(), memory_format=torch.channels_last)
    L.check(L.lib().unet_maxpool2_fwd(ops._DT[dtype], p(xd), n, h, w, c, p(out), st()), "maxpool fwd")
    assert torch.equal(out.double().cpu(), R.maxpool2(xq))
    dx = torch.full_like(xd, 7.0)
    L.check(L.lib().unet_maxpool2_bwd(ops._DT[dtype], p(xd), p(gpd), n, h, w, c, p(dx), 0, st()), "maxpool bwd")
    assert torch.equal(dx.double().cpu(), R.maxpool2_route(xq, R.rd(g, dtype)))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(1, 64, 1, 4), (2, 64, 5, 1), (1, 128, 1, 1), (2, 64, 5, 3), (2, 128, 128, 128),
                                   (2, 1024, 16, 16), (1, 64, 704, 256)], ids=str)
def test_bilinear2x(hip, dtype, shape):
    L, ops = hip
    n, c, h, w = shape
    x = activations(11000 + h, shape)
    xd = nhwc(x, dtype)
    y = torch.empty((n, c, 2 * h, 2 * w), dtype=dtype, device=dev(), memory_format=torch.channels_last)
    L.check(L.lib().unet_upsample_bilinear2x_fwd(ops._DT[dtype], p(xd), n, h, w, c, p(y), st()), "bilinear fwd")
    worst = {"y": cmp(dtype)(y, R.bilinear2x(x, dtype), f"bilinear fwd {shape}")}
    gy = activations(11001 + h, (n, c, 2 * h, 2 * w), sigma=1.0)
    dx = torch.empty((n, c, h, w), dtype=dtype, device=dev(), memory_format=torch.channels_last)
    gyd = nhwc(gy, dtype)
    L.check(L.lib().unet_upsample_bilinear2x_bwd(ops._DT[dtype], p(gyd), n, h, w, c, p(dx), st()), "bilinear bwd")
    worst["dx"] = cmp(dtype)(dx, R.bilinear2x_bwd(gy, dtype), f"bilinear bwd {shape}")
    report("unet_upsample_bilinear2x_fwd/_bwd", dtype, "x".join(map(str, shape)), **worst)


# ------------------------------------------------------------------ Adam
def _host_adam(decoupled, p0, g, m0, v0, step, wd):
    hp = torch.nn.Parameter(p0.clone())
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([hp], lr=1e-3, weight_decay=wd)
    opt.state[hp] = {"step": torch.tensor(float(step - 1)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
    hp.grad = g.clone()
    opt.step()
    return hp.detach(), opt.state[hp]["exp_avg"], opt.state[hp]["exp_avg_sq"]


@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
@pytest.mark.parametrize("steps", [(1, 2), (1000,)], ids=["steps1-2", "step1000"])
def test_adam_multi_every_element(hip, decoupled, steps):
    L, ops = hip
    import numpy as np
    chunk = L.lib().unet_adam_chunk_elems()
    sizes = [1, 3, 4, 5, 1023, chunk - 1, chunk, chunk + 1, 3 * chunk + 7]
    total = sum(sizes)
    wd = 1e-2
    p0, m0 = gen(12000, (total,)), gen(12001, (total,)) * 0.1
    v0 = gen(12002, (total,)) ** 2 * 0.01
    if steps[0] == 1:
        m0, v0 = torch.zeros(total), torch.zeros(total)
    grads = []
    for k in range(len(steps)):
        g = gen(12010 + k, (total,))
        g[::7], g[1::7], g[2::7] = 0.0, 1e-20, 1e4
        grads.append(g)
    # one arena per role; the LAST tensor starts 4 bytes into a 16-byte line (a slice of the arena), the others at
    # multiples of 16 bytes
    starts, at = [], 0
    for i, nel in enumerate(sizes):
        if i == len(sizes) - 1:
            at = (at + 3) // 4 * 4 + 1
        else:
            at = (at + 3) // 4 * 4
        starts.append(at)
        at += nel
    arena = at
    pd, md, vd, gd = (torch.zeros(arena + 4, device=dev()) for _ in range(4))
    assert pd.data_ptr() % 16 == 0 and (pd.data_ptr() + 4 * starts[-1]) % 16 == 4
    src, at = [], 0
    for s0, nel in zip(starts, sizes):
        src.append((s0, at, nel))
        at += nel

    def scatter(d, h):
        for s0, a0, nel in src:
            d[s0:s0 + nel] = h[a0:a0 + nel].to(dev())

    def gather(d):
        return torch.cat([d[s0:s0 + nel] for s0, _, nel in src]).cpu()
    scatter(pd, p0), scatter(md, m0), scatter(vd, v0)
    guard = [t.clone() for t in (pd, md, vd)]
    descs = torch.tensor([[t.data_ptr() + 4 * s0 for t in (pd, gd, md, vd)] + [nel] for s0, _, nel in src], dtype=torch.int64)
    rows = [(t, 0, first) for t, nel in enumerate(sizes) for first in range(0, nel, chunk)]
    ck = np.zeros(len(rows), dtype=[("tensor", "<i4"), ("reserved", "<i4"), ("first", "<i8")])
    for i, r in enumerate(rows):
        ck[i] = r
    dd, cd = descs.to(dev()), torch.from_numpy(ck.view(np.uint8).copy()).to(dev())
    ref = [(p0.double(), None), (m0.double(), None), (v0.double(), None)]
    host = (p0, m0, v0)
    for step, g in zip(steps, grads):
        scatter(gd, g)
        L.check(L.lib().unet_adam_multi(p(dd), p(cd), len(rows), 1e-3, 0.9, 0.999, 1e-8, wd, 1.0, step, int(decoupled), st()),
                "adam multi")
        ref = R.adam_step(ref[0][0], g, ref[1][0], ref[2][0], step, 1e-3, 0.9, 0.999, 1e-8, wd, decoupled)
        host = _host_adam(decoupled, host[0], g, host[1], host[2], step, wd)
    tag = f"{'adamw' if decoupled else 'adam'} steps {steps}"
    worst = {nm: R.assert_measured(gather(d), ref[i], host[i], f"{tag} {nm}") for i, (nm, d) in enumerate((("p", pd), ("m", md), ("v", vd)))}
    for nm in ("p", "m", "v"):
        hr, kr, al = R.MEASURED[f"{tag} {nm}"]
        print(f"\nREF64 measured unet_adam_multi {tag} {nm}: host err/S {hr:.3e} kernel err/S {kr:.3e} allowed {al:.3e}", flush=True)
    # nothing outside the tensors was written (the gaps of the arena)
    keep = torch.ones(arena + 4, dtype=torch.bool, device=dev())
    for s0, _, nel in src:
        keep[s0:s0 + nel] = False
    for d, g0 in zip((pd, md, vd), guard):
        assert torch.equal(d[keep], g0[keep]), "unet_adam_multi wrote outside its tensors"
    report("unet_adam_multi", "fp32", tag, **worst)


@pytest.mark.parametrize("step", [1, 1000])
def test_adam_step_every_element(hip, step):
    L, ops = hip
    n = 4 * 25000
    p0, g = gen(13000, (n,)), gen(13001, (n,))
    g[::7], g[1::7], g[2::7] = 0.0, 1e-20, 1e4
    m0, v0 = (torch.zeros(n), torch.zeros(n)) if step == 1 else (gen(13002, (n,)) * 0.1, gen(13003, (n,)) ** 2 * 0.01)
    pd, md, vd = p0.to(dev()), m0.to(dev()), v0.to(dev())
    ops.adam_step_(pd, g.to(dev()), md, vd, step, 1e-3, 0.9, 0.999, 1e-8, 1e-4)
    ref = R.adam_step(p0, g, m0, v0, step, 1e-3, 0.9, 0.999, 1e-8, 1e-4)
    host = _host_adam(False, p0, g, m0, v0, step, 1e-4)
    worst = {nm: R.assert_measured(d, ref[i], host[i], f"adam_step {step} {nm}") for i, (nm, d) in enumerate((("p", pd), ("m", md), ("v", vd)))}
    for nm in ("p", "m", "v"):
        hr, kr, al = R.MEASURED[f"adam_step {step} {nm}"]
        print(f"\nREF64 measured unet_adam_step step {step} {nm}: host err/S {hr:.3e} kernel err/S {kr:.3e} allowed {al:.3e}", flush=True)
    report("unet_adam_step", "fp32", f"step {step}", **worst)


# ------------------------------------------------------------------ anomaly score, MSE + focal loss
LOSS_PIXELS = SWEEP_PIXELS + [32 * 256 * 256, 2 * 1408 * 512]


@pytest.mark.parametrize("hw", SWEEP_PIXELS + [256 * 256, 1408 * 512])
def test_anomaly_score(hip, hw):
    L, ops = hip
    n = 32 if hw == 256 * 256 else 2
    recon, image = gen(14000 + hw % 997, (n, 3, hw)) + 0.5, gen(14001 + hw % 997, (n, 3, hw))
    rd_, id_ = recon.to(dev()), image.to(dev())
    need = L.lib().unet_anomaly_score_workspace(n, hw)
    ws = torch.empty(need, dtype=torch.uint8, device=dev())
    worst = {}
    for l1 in (0, 1):
        score, img = torch.empty(n, hw, device=dev()), torch.empty(n, device=dev())
        L.check(L.lib().unet_anomaly_score(p(rd_), p(id_), n, 3, hw, l1, p(score), p(img), p(ws), need, st()), "anomaly score")
        rs, ri = R.anomaly_score(recon, image, bool(l1))
        worst[f"score_l{2 - l1}"] = R.assert_fp32(score, rs, f"anomaly score hw={hw} l1={l1}")
        worst[f"image_l{2 - l1}"] = R.assert_fp32(img, ri, f"image score hw={hw} l1={l1}")
    report("unet_anomaly_score", "fp32", f"n={n},hw={hw}", **worst)


LOSS_CASES = [(px, 2.0) for px in LOSS_PIXELS] + [(px, 1.5) for px in SWEEP_PIXELS + [70001]]     # powf path: up to 70 001


@pytest.mark.parametrize("pixels,gamma", LOSS_CASES, ids=[f"pixels={px}-gamma={g}" for px, g in LOSS_CASES])
def test_mse_focal_loss(hip, pixels, gamma):
    """pixels = elements of the anomaly map; the reconstruction has 3 x as many.  The edge probabilities 0, 1, 1e-30,
    1 - 1e-7, 0.5 and a denormal lead the map at every size.  gamma = 2 is the kernel's square path (all sizes up to
    (32, 1, 256, 256) and (2, 1, 1408, 512) maps), 1.5 its powf path."""
    from oracle import unet_oracle as O
    L, ops = hip
    recon, image = gen(15000, (3 * pixels,), "uniform"), gen(15001, (3 * pixels,))
    amap = gen(15002, (pixels,), "uniform")
    edge = torch.tensor([0.0, 1.0, 1e-30, 1 - 1e-7, 0.5, 1e-45])[:pixels]
    amap[:edge.numel()] = edge
    mask = (gen(15003, (pixels,), "uniform") < 0.1).float()
    dv = [t.to(dev()) for t in (recon, image, amap, mask)]
    losses, d_recon, d_amap = torch.empty(2, device=dev()), torch.empty(3 * pixels, device=dev()), torch.empty(pixels, device=dev())
    need = L.lib().unet_loss_workspace(3 * pixels)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev())
    L.check(L.lib().unet_loss_mse_focal(p(dv[0]), p(dv[1]), 3 * pixels, p(dv[2]), p(dv[3]), pixels, 0.25, gamma, p(losses),
                                        p(d_recon), p(d_amap), p(ws), need, st()), "mse focal")
    ref = R.mse_focal(recon, image, amap, mask, 0.25, gamma)
    rr, ar = recon.clone().requires_grad_(True), amap.clone().requires_grad_(True)        # the oracle in fp32 on the host
    host = O.combined_loss(rr, ar, image, mask, focal_gamma=gamma)
    host["total_loss"].backward()
    tag = f"mse_focal pixels={pixels} gamma={gamma}"
    assert bool(torch.isfinite(d_amap).all())
    worst = {"mse": R.assert_fp32(losses[0], ref["mse"], tag + " mse"),
             "d_recon": R.assert_fp32(d_recon, ref["d_recon"], tag + " d_recon"),
             "focal": R.assert_measured(losses[1], ref["focal"], host["seg_loss"].detach(), tag + " focal", extra=R.SUM_EPS),
             "d_amap": R.assert_measured(d_amap, ref["d_amap"], ar.grad, tag + " d_amap")}
    for nm in ("focal", "d_amap"):
        hr, kr, al = R.MEASURED[f"{tag} {nm}"]
        print(f"\nREF64 measured unet_loss_mse_focal pixels={pixels} gamma={gamma} {nm}: host err/S {hr:.3e} kernel err/S {kr:.3e} "
              f"allowed {al:.3e}", flush=True)
    report("unet_loss_mse_focal", "fp32", f"pixels={pixels},gamma={gamma}", **worst)


# ------------------------------------------------------------------ 1x1 head
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("co", [1, 3, 4, 8])
@pytest.mark.parametrize("sigmoid", [False, True], ids=["logits", "sigmoid"])
@pytest.mark.parametrize("frame", [(2, 9, 11), (1, 1, 1), (2, 256, 256), (1, 1408, 512)], ids=str)
def test_head(hip, dtype, co, sigmoid, frame):
    L, ops = hip
    n, h, w = frame
    ci = 64
    x = activations(16000 + h, (n, ci, h, w), offset=0.2, sigma=1.0).clamp_min(0)         # post-ReLU activations
    wt, b = gen(16001 + co, (co, ci, 1, 1)) * 0.2, gen(16002 + co, (co,)) * 0.5
    xd, wd, bd = nhwc(x, dtype), wt.to(dev()), b.to(dev())
    out = torch.empty(n, co, h, w, device=dev())
    L.check(L.lib().unet_head_fwd(ops._DT[dtype], p(xd), n, h, w, ci, p(wd), p(bd), co, int(sigmoid), p(out), st()), "head fwd")
    ref = R.head_fwd(x, dtype, wt, b, sigmoid)
    tag = f"head co={co} sigmoid={sigmoid} {frame}"
    worst = {}
    if sigmoid:
        host = torch.sigmoid(F.conv2d(R.rd(x, dtype).float(), wt, b))
        worst["out"] = R.assert_measured(out, ref, host, tag + " out", extra=R.SUM_EPS)
        hr, kr, al = R.MEASURED[tag + " out"]
        print(f"\nREF64 measured unet_head_fwd sigmoid {IDS[DTYPES.index(dtype)]} co={co} {frame}: host err/S {hr:.3e} kernel err/S "
              f"{kr:.3e} allowed {al:.3e}", flush=True)
    else:
        worst["out"] = R.assert_fp32(out, ref, tag + " out")
    # backward on the test's own operands: the forward result rounded to fp32 from float64, a random gradient
    o32 = ref[0].float()
    dout = gen(16003 + co, (n, co, h, w)) + 0.5
    od, gd = o32.to(dev()), dout.to(dev())
    dx = torch.empty_like(xd)
    dw, db = torch.empty(co, ci, 1, 1, device=dev()), torch.empty(co, device=dev())
    need = L.lib().unet_head_bwd_workspace(n, h, w, ci, co)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev())
    L.check(L.lib().unet_head_bwd(ops._DT[dtype], p(xd), p(od), p(gd), n, h, w, ci, p(wd), co, int(sigmoid), p(dx), p(dw), p(db),
                                  p(ws), need, st()), "head bwd")
    bw = R.head_bwd(x, dtype, o32, dout, wt, sigmoid)
    worst["dx"] = cmp(dtype)(dx, bw["dx"], tag + " dx")
    worst["dW"] = R.assert_fp32(dw, bw["dw"], tag + " dW")
    worst["db"] = R.assert_fp32(db, bw["db"], tag + " db")
    report("unet_head_fwd/_bwd", dtype, f"co={co},sigmoid={int(sigmoid)},{n}x{h}x{w}", **worst)


# ------------------------------------------------------------------ 1x1 head reading the raw conv output (BatchNorm + ReLU on load)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("co", [1, 3, 4, 8])
@pytest.mark.parametrize("sigmoid", [False, True], ids=["logits", "sigmoid"])
@pytest.mark.parametrize("frame", [(2, 9, 11), (1, 1, 1), (2, 256, 256), (1, 1408, 512)], ids=str)
def test_head_fused_with_batchnorm_relu(hip, dtype, co, sigmoid, frame):
    L, ops = hip
    n, h, w = frame
    ci = 64
    gamma, mean, istd, scale, shift = coefficients(17000 + co, ci)
    y = activations(17001 + h, (n, ci, h, w))
    y[:, 1] = 0.0                                          # exact zeros at the ReLU of channel 1
    shift[1] = 0.0
    wt, b = gen(17002 + co, (co, ci, 1, 1)) * 0.2, gen(17003 + co, (co,)) * 0.5
    yd, wd, bd = nhwc(y, dtype), wt.to(dev()), b.to(dev())
    sd, hd, md = scale.to(dev()), shift.to(dev()), mean.to(dev())
    out = torch.empty(n, co, h, w, device=dev())
    dt = ops._DT[dtype]
    L.check(L.lib().unet_head_bnrelu_fwd(dt, p(yd), n, h, w, ci, p(sd), p(hd), p(wd), p(bd), co, int(sigmoid), p(out), st()),
            "head bnrelu fwd")
    ref = R.head_bnrelu_fwd(y, dtype, scale, shift, wt, b, sigmoid)
    tag = f"fused head co={co} sigmoid={sigmoid} {frame} {IDS[DTYPES.index(dtype)]}"
    worst = {}
    if sigmoid:
        a32 = R.stored(R.bn_relu_apply(y, dtype, scale, shift)[0], dtype).float()
        host = torch.sigmoid(F.conv2d(a32, wt, b))
        worst["out"] = R.assert_measured(out, ref, host, tag + " out", extra=R.SUM_EPS)
        hr, kr, al = R.MEASURED[tag + " out"]
        print(f"\nREF64 measured unet_head_bnrelu_fwd sigmoid {IDS[DTYPES.index(dtype)]} co={co} {frame}: host err/S {hr:.3e} "
              f"kernel err/S {kr:.3e} allowed {al:.3e}", flush=True)
    else:
        worst["out"] = R.assert_fp32(out, ref, tag + " out")
    o32 = ref[0].float()
    dout = gen(17004 + co, (n, co, h, w)) + 0.5
    od, gd = o32.to(dev()), dout.to(dev())
    dz = torch.empty_like(yd)
    dw, db = torch.empty(co, ci, 1, 1, device=dev()), torch.empty(co, device=dev())
    cap = L.lib().unet_head_bnrelu_max_parts()
    part = torch.zeros(cap, 2, ci, device=dev())
    nparts = C.c_int32(0)
    need = L.lib().unet_head_bwd_workspace(n, h, w, ci, co)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev())
    L.check(L.lib().unet_head_bnrelu_bwd(dt, p(yd), p(sd), p(hd), p(md), p(od), p(gd), n, h, w, ci, p(wd), co, int(sigmoid), p(dz),
                                         p(dw), p(db), p(part), C.byref(nparts), p(ws), need, st()), "head bnrelu bwd")
    assert 0 < nparts.value <= cap
    bw = R.head_bnrelu_bwd(y, dtype, scale, shift, mean, o32, dout, wt, sigmoid)
    worst["dz"] = cmp(dtype)(dz, bw["dz"], tag + " dz")
    assert float(dz[:, 1].abs().max()) == 0            # z = 0 exactly: masked
    worst["dW"] = R.assert_fp32(dw, bw["dw"], tag + " dW")
    worst["db"] = R.assert_fp32(db, bw["db"], tag + " db")
    # the partials are sums over the dz the kernel stored (the operand unet_bn_bwd_premasked reads next)
    dzk = dz.double().cpu()
    t = dzk * (R.rd(y, dtype) - R._c(mean))
    sums = part[:nparts.value].double().sum(0).cpu()
    worst["sum"] = R.assert_fp32(sums[0], (dzk.sum((0, 2, 3)), dzk.abs().sum((0, 2, 3))), tag + " sum dz")
    worst["sum_c"] = R.assert_fp32(sums[1], (t.sum((0, 2, 3)), t.abs().sum((0, 2, 3))), tag + " sum dz (y - mean)")
    report("unet_head_bnrelu_fwd/_bwd", dtype, f"co={co},sigmoid={int(sigmoid)},{n}x{h}x{w}", **worst)


# ------------------------------------------------------------------ SSIM
SSIM_CASES = [(1, 1, 1, 1), (1, 1, 5, 300), (1, 3, 31, 33), (2, 3, 32, 32), (1, 1, 65, 7), (3, 2, 100, 129), (2, 3, 250, 203),
              (2, 3, 1408, 512), (32, 3, 256, 256)]


# the two largest run once each (mean over the batch / per image) to bound the float64 host time
SSIM_RUNS = [(cs, pi) for cs in SSIM_CASES for pi in (False, True)
             if (cs, pi) not in (((32, 3, 256, 256), True), ((2, 3, 1408, 512), False))]


@pytest.mark.parametrize("case,per_image", SSIM_RUNS, ids=[f"{cs}-{'per_image' if pi else 'mean'}" for cs, pi in SSIM_RUNS])
def test_ssim_loss(hip, case, per_image):
    """frames below, at and across the 32-pixel tile (1 to 768 block partials per call), the benchmark batch and the
    1408 x 512 frame"""
    from oracle import unet_oracle as O
    L, ops = hip
    n, c, h, w = case
    a, b = gen(18000 + h, case, "uniform"), gen(18001 + h, case) * 0.5 + 0.5
    ad, bd = a.to(dev()), b.to(dev())
    loss = torch.empty(n if per_image else 1, device=dev())
    d1, d2 = torch.empty_like(ad), torch.empty_like(bd)
    planes = c if per_image else n * c
    need = L.lib().unet_ssim_workspace(planes, h, w)
    ws = torch.empty(need, dtype=torch.uint8, device=dev())
    if per_image:
        L.check(L.lib().unet_ssim_loss_per_image(p(ad), p(bd), n, c, h, w, 11, p(loss), p(d1), p(d2), p(ws), need, st()), "ssim per image")
    else:
        L.check(L.lib().unet_ssim_loss(p(ad), p(bd), n * c, h, w, 11, p(loss), p(d1), p(d2), p(ws), need, st()), "ssim")
    ref = R.ssim(a, b, 11, per_image)
    ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)           # the oracle in fp32 on the host
    hv = O.ssim_loss(ar, br, 11, size_average=not per_image)
    hv.sum().backward()
    tag = f"ssim {case} {'per image' if per_image else 'mean'}"
    worst = {"loss": R.assert_measured(loss.view(ref["loss"][0].shape), ref["loss"], hv.detach(), tag + " loss", extra=R.SUM_EPS),
             "d_img1": R.assert_measured(d1, ref["d1"], ar.grad, tag + " d_img1"),
             "d_img2": R.assert_measured(d2, ref["d2"], br.grad, tag + " d_img2")}
    entry = "unet_ssim_loss_per_image" if per_image else "unet_ssim_loss"
    for nm in ("loss", "d_img1", "d_img2"):
        hr, kr, al = R.MEASURED[f"{tag} {nm}"]
        print(f"\nREF64 measured {entry} {case} {nm}: host err/S {hr:.3e} kernel err/S {kr:.3e} allowed {al:.3e}", flush=True)
    report(entry, "fp32", "x".join(map(str, case)), **worst)


# ------------------------------------------------------------------ statistics finalized from the conv epilogues' partials
def _finalize(L, part, nparts, pixels, c, gamma, beta, rm, rv, momentum):
    out = torch.empty(4, c, device=dev())
    gd, bd = gamma.to(dev()), beta.to(dev())
    rmd, rvd = (None, None) if rm is None else (rm.to(dev()).clone(), rv.to(dev()).clone())
    L.check(L.lib().unet_bn_finalize_partials(p(part), nparts, pixels, c, p(gd), p(bd), p(rmd), p(rvd), momentum, EPS, p(out[0]),
                                              p(out[1]), p(out[2]), p(out[3]), st()), "finalize partials")
    got = {"mean": out[0], "istd": out[1], "scale": out[2], "shift": out[3]}
    if rm is not None:
        got["running_mean"], got["running_var"] = rmd, rvd
    return got


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", [(2, 64, 64, 24, 40), (1, 64, 128, 9, 21), (3, 256, 128, 8, 8), (4, 64, 64, 128, 144),
                                  (40, 64, 64, 64, 64), (6, 64, 64, 200, 136), (8, 64, 64, 256, 256)], ids=str)
def test_bn_finalize_partials_after_conv3x3_stats(hip, dtype, case):
    """unet_conv3x3_stats leaves per-channel partial sums of the y it STORED; unet_bn_finalize_partials on them must give the
    statistics of that y within the bounds of bn_train_stats (both finalize shapes: fewer and more than 128 partials)"""
    L, ops = hip
    n, ci, co, h, w = case
    x = activations(19000 + h, (n, ci, h, w), offset=0.5, sigma=1.0)
    wt = gen(19001 + co, (co, ci, 3, 3)) * (1.0 / (3 * ci ** 0.5))
    xd = nhwc(x, dtype)
    y = ops._nhwc_empty(n, co, h, w, dtype, dev())
    wp = ops.pack_weight(wt.to(dev()), L.PACK_CONV_FWD, co, ci, dtype)
    cap = L.lib().unet_conv3x3_stats_max_parts(n, h, w)
    part = torch.full((cap, 2, co), float("nan"), device=dev())
    nparts = C.c_int32(0)
    src = L.View2()
    src[0] = L.View(xd.data_ptr(), ci, h, w, 0, 0)
    src[1] = L.View(None, 0, 0, 0, 0, 0)
    L.check(L.lib().unet_conv3x3_stats(ops._DT[dtype], n, h, w, src, p(wp), co, p(y), p(part), C.byref(nparts), st()), "conv+stats")
    assert 0 < nparts.value <= cap
    gamma, beta = gen(1, (co,), "uniform") + 0.5, gen(2, (co,)) * 0.3
    rm, rv = gen(3, (co,)) * 0.1, gen(4, (co,), "uniform") + 0.5
    yk = y.float().cpu()
    worst = {}
    for momentum, r_m, r_v in ((0.1, rm, rv), (0.25, rm, rv), (0.1, None, None)):
        got = _finalize(L, part, nparts.value, n * h * w, co, gamma, beta, r_m, r_v, momentum)
        ref = R.bn_train_stats(yk, dtype, gamma, beta, r_m, r_v, momentum, EPS)
        for k, v in check_stats(got, ref, f"finalize {case} m={momentum}").items():
            worst[k] = max(worst.get(k, 0.0), v)
    report("unet_conv3x3_stats + unet_bn_finalize_partials", dtype, f"{case} n_parts={nparts.value}".replace(" ", ""), **worst)


@pytest.mark.parametrize("case", [(2, 3, 12, 32), (1, 1, 16, 16), (3, 3, 33, 48), (8, 3, 256, 256), (2, 3, 1408, 512)], ids=str)
def test_bn_finalize_partials_after_first_layer_stats(hip, case):
    L, ops = hip
    n, ci, h, w = case
    co = 64
    assert L.lib().unet_conv3x3_first_supported(ci, co, h, w)
    x = gen(19100 + h, (n, ci, h, w)) + 0.3
    wt = gen(19101, (co, ci, 3, 3)) * 0.2
    xd, wd = x.to(dev()), wt.to(dev())
    y = ops._nhwc_empty(n, co, h, w, torch.bfloat16, dev())
    cap = L.lib().unet_conv3x3_stats_max_parts(n, h, w)
    part = torch.full((cap, 2, co), float("nan"), device=dev())
    nparts = C.c_int32(0)
    L.check(L.lib().unet_conv3x3_first_stats(n, h, w, p(xd), ci, p(wd), p(y), p(part), C.byref(nparts), st()), "first conv+stats")
    assert 0 < nparts.value <= cap
    gamma, beta = gen(1, (co,), "uniform") + 0.5, gen(2, (co,)) * 0.3
    rm, rv = gen(3, (co,)) * 0.1, gen(4, (co,), "uniform") + 0.5
    got = _finalize(L, part, nparts.value, n * h * w, co, gamma, beta, rm, rv, 0.1)
    worst = check_stats(got, R.bn_train_stats(y.float().cpu(), torch.bfloat16, gamma, beta, rm, rv, 0.1, EPS), f"first-layer finalize {case}")
    report("unet_conv3x3_first_stats + unet_bn_finalize_partials", torch.bfloat16, f"{case} n_parts={nparts.value}".replace(" ", ""), **worst)
