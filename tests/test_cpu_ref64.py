"""CPU self-test of tests/_ref64.py: the exact reference passes its own comparator, and the defects the bf16 GPU tests
are there to catch -- one dropped product term, truncating instead of round-to-nearest-even, one missing 32-pixel
block of a weight-gradient reduction at the largest K the suite uses -- are rejected.  The second half does the same for
the references of the streaming and reduction kernels (BatchNorm, pooling, bilinear, Adam), the last part for the
segmentation loss (seg_loss): torch's float64 operators and autograd agree with the closed forms, and a missing block
partial, a missing tail pixel, wrong Dice coefficients, a dropped focal derivative term, a clamped cross entropy and the
two contract slips (Dice sum p skipping ignored pixels, focal averaged over valid pixels) are rejected.  At the end the
folded-BatchNorm inference convolution (conv3x3_bias_relu): an fp32-accumulating emulation passes, a shift from the wrong
channel, a misplaced or missing ReLU, the neighbouring row's scale, a bf16-rounded shift and a truncating store do not.
Last, the fp32 compute dtype of the convolution references (test_gpu_staged.py): fp32 host results on unrounded operands
pass 2^-18 S; operands narrowed to bf16 or 10 mantissa bits, a zeroed tap, a missing 8 x 16 pixel tile of a weight
gradient and an accumulate that drops the old value do not."""
import pytest
import torch

import _ref64 as R


def _gen(seed, shape):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64)


def _as_kernel_bf16(v):
    """what a correct kernel stores: the exact value rounded to nearest-even in bf16"""
    return v.to(torch.float32).to(torch.bfloat16)


@pytest.fixture(scope="module")
def conv1024():
    x = _gen(1, (1, 1024, 6, 5))
    w = _gen(2, (64, 1024, 3, 3)) / (3 * 1024 ** 0.5)
    return x, w, R.conv3x3(x, w)


def test_exact_reference_is_accepted(conv1024):
    x, w, rs = conv1024
    assert R.assert_bf16(_as_kernel_bf16(rs[0]), rs, "exact conv") <= 1.0
    dw = R.conv3x3_wgrad(x, _gen(3, (1, 64, 6, 5)))
    assert R.assert_fp32(dw[0].to(torch.float32), dw, "exact wgrad") <= 1.0
    xt, wt, b = _gen(4, (3, 128, 5, 7)), _gen(5, (128, 64, 2, 2)) * 0.1, _gen(6, (64,)).float()
    y = R.convt2x2(xt, wt, b)
    R.assert_bf16(_as_kernel_bf16(y[0]), y, "exact convT")
    (dwt, db) = R.convt2x2_wgrad(xt, _gen(7, (3, 64, 10, 14)))
    R.assert_fp32(dwt[0].float(), dwt, "exact convT wgrad")
    R.assert_fp32(db[0].float(), db, "exact convT bias grad")


def test_convt_references_match_autograd():
    x, w, b = _gen(8, (2, 128, 3, 5)), _gen(9, (128, 64, 2, 2)), _gen(10, (64,))
    gy = _gen(11, (2, 64, 6, 10))
    xq, wq = R.q64(x).requires_grad_(True), R.q64(w).requires_grad_(True)
    bq = b.float().double().requires_grad_(True)          # (the bias is an fp32 operand)
    y = torch.nn.functional.conv_transpose2d(xq, wq, bq, stride=2)
    y.backward(R.q64(gy))
    assert torch.allclose(R.convt2x2(x, w, b.float())[0], y, rtol=1e-12, atol=1e-12)
    assert torch.allclose(R.convt2x2_dgrad(gy, w)[0], xq.grad, rtol=1e-12, atol=1e-12)
    (dw, db) = R.convt2x2_wgrad(x, gy)
    assert torch.allclose(dw[0], wq.grad, rtol=1e-12, atol=1e-12) and torch.allclose(db[0], bq.grad, rtol=1e-12, atol=1e-12)


def test_one_dropped_product_term_is_rejected(conv1024):
    """1024-channel 3x3 conv: drop the largest of the 9216 product terms of one element whose |ref| is the median"""
    x, w, (ref, S) = conv1024
    flat = ref.abs().view(-1)
    i = int(flat.argsort()[flat.numel() // 2])
    n, co, yy, xx = R._where(i, tuple(ref.shape))
    xp = torch.nn.functional.pad(R.q64(x), [1, 1, 1, 1])
    terms = xp[n, :, yy:yy + 3, xx:xx + 3] * R.q64(w)[co]
    k = int(terms.abs().argmax())
    bad = ref.clone()
    bad[n, co, yy, xx] -= terms.view(-1)[k]
    with pytest.raises(AssertionError, match=rf"\({n}, {co}, {yy}, {xx}\)"):
        R.assert_bf16(_as_kernel_bf16(bad), (ref, S), "dropped term")


def test_truncating_epilogue_is_rejected(conv1024):
    _, _, rs = conv1024
    with pytest.raises(AssertionError):
        R.assert_bf16(R.round_bf16_toward_zero(rs[0]), rs, "truncating store")
    # the exact value truncated to fp32 is fine: only the bf16 rounding direction is at issue
    R.assert_bf16(_as_kernel_bf16(rs[0].to(torch.float32).double()), rs, "fp32 then rne")


def test_missing_split_k_block_is_rejected_at_the_largest_wgrad_k():
    """one 32-pixel block of the K = N*H*W reduction missing from one weight-gradient element, at the largest K of the
    suite's bf16 weight-gradient comparisons (the split-K slab a narrow reduce could skip)"""
    n, h, w = 8, 128, 128
    assert n * h * w == R.MAX_WGRAD_K
    ci, co = 2, 2            # the bound scales with K, not with the channel counts
    x, dy = _gen(12, (n, ci, h, w)), _gen(13, (n, co, h, w))
    ref, S = R.conv3x3_wgrad(x, dy)
    R.assert_fp32(ref.to(torch.float32), (ref, S), "exact wgrad at max K")
    flat = ref.abs().view(-1)
    i = int(flat.argsort()[flat.numel() // 2])
    o, c, ky, kx = R._where(i, tuple(ref.shape))
    xp = torch.nn.functional.pad(R.q64(x), [1, 1, 1, 1])
    terms = (R.q64(dy)[:, o] * xp[:, c, ky:ky + h, kx:kx + w]).reshape(-1)       # the K terms in (n, y, x) order
    blocks = terms.view(-1, 32).sum(1)
    b = int(blocks.abs().argsort()[blocks.numel() // 2])          # a block of median weight: no cherry-picking
    bad = ref.clone()
    bad[o, c, ky, kx] -= blocks[b]
    with pytest.raises(AssertionError, match=rf"\({o}, {c}, {ky}, {kx}\)"):
        R.assert_fp32(bad.to(torch.float32), (ref, S), "missing K block")


def test_half_ulp_is_exact():
    v = torch.tensor([1.0, 1.5, 2.0, 0.75, -3.0, 2.0 ** -20, 0.0], dtype=torch.float64)
    want = torch.tensor([2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9, 2.0 ** -7, 2.0 ** -28, 0.0], dtype=torch.float64)
    assert torch.equal(R.half_ulp_bf16(v), want)
    # a correct round-to-nearest-even of any value lands within it
    u = _gen(14, (10000,)) * 100
    assert bool(((u.float().bfloat16().double() - u).abs() <= R.half_ulp_bf16(u) + 2.0 ** -24 * u.abs()).all())     # (+ the fp32 step)


# ====================================================================== streaming / reduction kernels
# (BatchNorm, pooling, bilinear, Adam): the references equal torch in float64, the exact value stored the way a correct
# kernel stores it passes, and each planted defect is rejected at the largest size the GPU tests use it at.
F = torch.nn.functional
EPS32 = float(torch.tensor(1e-5, dtype=torch.float32))
F64 = torch.float64


def _close(a, b):
    return torch.allclose(a, b, rtol=1e-12, atol=1e-12)


def _bn_case(seed, shape, offset=0.3):
    c = shape[1]
    y = _gen(seed, shape) * 1.7 + offset
    ga, be = torch.rand(c, generator=torch.Generator().manual_seed(seed + 1), dtype=F64) + 0.5, _gen(seed + 2, (c,)) * 0.3
    rm, rv = _gen(seed + 3, (c,)) * 0.1, torch.rand(c, generator=torch.Generator().manual_seed(seed + 4), dtype=F64) + 0.5
    return y, ga, be, rm, rv, _gen(seed + 5, shape)


@pytest.mark.parametrize("momentum", [0.1, 1.0 / 3.0])          # (momentum=None: the caller passes 1 / batches seen)
def test_bn_references_match_autograd(momentum):
    y, ga, be, rm, rv, da = _bn_case(20, (3, 8, 7, 5))
    m32 = float(torch.tensor(momentum, dtype=torch.float32))
    yr, gr, br = y.clone().requires_grad_(True), ga.clone().requires_grad_(True), be.clone().requires_grad_(True)
    trm, trv = rm.clone(), rv.clone()
    a = F.relu(F.batch_norm(yr, trm, trv, gr, br, True, m32, EPS32))
    a.backward(da)
    st = R.bn_train_stats(y, F64, ga, be, rm, rv, momentum, 1e-5)
    assert _close(st["mean"][0], y.mean((0, 2, 3))) and _close(st["var"][0], y.var((0, 2, 3), unbiased=False))
    assert _close(st["running_mean"][0], trm) and _close(st["running_var"][0], trv)
    scale, shift, mean, istd = st["scale"][0], st["shift"][0], st["mean"][0], st["istd"][0]
    assert _close(R.bn_relu_apply(y, F64, scale, shift)[0], a.detach())
    bw = R.bn_relu_bwd(da, y, F64, ga, mean, istd, scale, shift)
    assert _close(bw["dbeta"][0], br.grad) and _close(bw["dgamma"][0], gr.grad) and _close(bw["dy"][0], yr.grad)
    # frozen statistics (eval-mode BatchNorm inside a training graph) and the eval coefficients
    yr2, gr2, br2 = y.clone().requires_grad_(True), ga.clone().requires_grad_(True), be.clone().requires_grad_(True)
    a2 = F.relu(F.batch_norm(yr2, rm, rv, gr2, br2, False, 0.0, EPS32))
    a2.backward(da)
    ev = R.bn_eval_coeffs(ga, be, rm, rv)
    assert _close(R.bn_relu_apply(y, F64, ev["scale"][0], ev["shift"][0])[0], a2.detach())
    fz = R.bn_relu_bwd(da, y, F64, ga, ev["mean"][0], ev["istd"][0], ev["scale"][0], ev["shift"][0], frozen=True)
    assert _close(fz["dbeta"][0], br2.grad) and _close(fz["dgamma"][0], gr2.grad) and _close(fz["dy"][0], yr2.grad)


def test_single_pixel_statistics_are_finite():
    y, ga, be, rm, rv, _ = _bn_case(26, (1, 4, 1, 1))
    st = R.bn_train_stats(y, F64, ga, be, rm, rv)
    assert torch.equal(st["var"][0], torch.zeros(4, dtype=F64)) and _close(st["istd"][0], torch.full((4,), EPS32 ** -0.5, dtype=F64))
    assert _close(st["running_var"][0], (1 - float(torch.tensor(0.1, dtype=torch.float32))) * rv) and bool(torch.isfinite(st["running_var"][0]).all())


def test_pool_and_bilinear_references_match_autograd():
    x = _gen(30, (2, 3, 7, 9)).bfloat16().double()
    x[:, 0, 0:2, 0:2] = 1.5                                       # ties: first maximum
    g = _gen(31, (2, 3, 3, 4)).bfloat16().double()
    xr = x.clone().requires_grad_(True)
    yp = F.max_pool2d(xr, 2)
    yp.backward(g)
    assert torch.equal(R.maxpool2(x), yp.detach()) and torch.equal(R.maxpool2_route(x, g), xr.grad)
    assert float(R.maxpool2_route(x, g)[:, :, 6].abs().max()) == 0 and float(R.maxpool2_route(x, g)[:, :, :, 8].abs().max()) == 0
    # fused BatchNorm + ReLU + pool backward, scale 1 / shift 0 on bf16-grid data in fp32: every store is exact
    old = _gen(32, (2, 3, 7, 9)).bfloat16().double()
    one, zero = torch.ones(3), torch.zeros(3)
    xr = x.clone().requires_grad_(True)
    ar = F.relu(xr)
    (F.max_pool2d(ar, 2) * g).sum().backward(retain_graph=True)
    ar.backward(old)
    pb = R.bn_relu_pool_bwd(x, g, old, torch.float32, one, zero, zero)
    assert _close(pb["dz"][0], xr.grad) and _close(pb["dz_stored"], xr.grad)
    assert _close(pb["sum"][0], xr.grad.sum((0, 2, 3))) and _close(pb["sum_c"][0], (xr.grad * x).sum((0, 2, 3)))
    for shape in ((2, 3, 5, 4), (1, 2, 1, 6), (1, 2, 3, 1)):
        u = _gen(33, shape)
        ur = u.clone().requires_grad_(True)
        up = F.interpolate(ur, scale_factor=2, mode="bilinear", align_corners=True)
        gy = _gen(34, tuple(up.shape))
        up.backward(gy)
        assert _close(R.bilinear2x(u, F64)[0], up.detach()) and _close(R.bilinear2x_bwd(gy, F64)[0], ur.grad)


@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_adam_reference_matches_torch_optim(decoupled):
    p0, g1, g2 = _gen(40, (257,)), _gen(41, (257,)), _gen(42, (257,))
    lr, eps, wd = (float(torch.tensor(x, dtype=torch.float32)) for x in (1e-3, 1e-8, 1e-2))
    ref = torch.nn.Parameter(p0.clone())
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([ref], lr=lr, eps=eps, weight_decay=wd)
    p, m, v = p0, torch.zeros_like(p0), torch.zeros_like(p0)
    for step, g in enumerate((g1, g2), 1):
        ref.grad = g.clone()
        opt.step()
        (p, _), (m, _), (v, _) = R.adam_step(p, g, m, v, step, 1e-3, 0.9, 0.999, 1e-8, 1e-2, decoupled)
    assert _close(p, ref.detach()) and _close(m, opt.state[ref]["exp_avg"]) and _close(v, opt.state[ref]["exp_avg_sq"])


# ---------------------------------------------------------------------- exact values pass, planted defects do not
@pytest.fixture(scope="module")
def stream_case():
    """bf16-grid data of the GPU tests' generator: 1.7 randn + 0.3, scale in [0.5, 1.5), shift = 0.3 randn; exact zeros
    and negative zeros planted in channel 0 (with shift[0] = 0 the pre-activation there is exactly 0)"""
    y, ga, be, rm, rv, da = _bn_case(50, (4, 8, 64, 64))
    y = y.bfloat16().double()
    y[:, 0, ::2, ::3] = 0.0
    y[:, 0, 1::2, ::3] = -0.0
    scale, shift = ga.float(), (be * 1.0).float()
    shift[0] = 0.0
    return y, da.bfloat16().double(), scale, shift


def test_exact_streaming_values_are_accepted(stream_case):
    y, da, scale, shift = stream_case
    for dt in (torch.bfloat16, torch.float32):
        a = R.bn_relu_apply(y, dt, scale, shift)
        (R.assert_bf16 if dt == torch.bfloat16 else R.assert_fp32)(R.stored(a[0], dt), a, "exact bn apply")
    mean, istd = _gen(51, (8,)).float() * 0.1, (torch.rand(8) + 0.5)
    bw = R.bn_relu_bwd(da, y, torch.bfloat16, scale / istd, mean, istd, scale, shift)
    R.assert_bf16(_as_kernel_bf16(bw["dy"][0]), bw["dy"], "exact bn dy", mask=bw["clear"])
    assert float((~bw["clear"]).double().mean()) <= 1e-3
    R.assert_fp32(bw["dbeta"][0].float(), bw["dbeta"], "exact dbeta")
    R.assert_fp32(bw["dgamma"][0].float(), bw["dgamma"], "exact dgamma")
    up = R.bilinear2x(y, torch.bfloat16)
    R.assert_bf16(_as_kernel_bf16(up[0]), up, "exact bilinear")
    st = R.bn_train_stats(y, torch.bfloat16, scale, shift, mean, istd)
    for k in ("mean", "istd", "scale", "shift", "running_mean", "running_var"):
        R.assert_fp32(st[k][0].float(), st[k], "exact " + k)


def test_truncating_streaming_stores_are_rejected(stream_case):
    y, da, scale, shift = stream_case
    a = R.bn_relu_apply(y, torch.bfloat16, scale, shift)
    with pytest.raises(AssertionError):
        R.assert_bf16(R.round_bf16_toward_zero(a[0]), a, "truncated bn apply")
    up = R.bilinear2x(y, torch.bfloat16)
    with pytest.raises(AssertionError):
        R.assert_bf16(R.round_bf16_toward_zero(up[0]), up, "truncated bilinear")
    dn = R.bilinear2x_bwd(da, torch.bfloat16)
    with pytest.raises(AssertionError):
        R.assert_bf16(R.round_bf16_toward_zero(dn[0]), dn, "truncated bilinear adjoint")


def test_wrong_relu_masks_are_rejected(stream_case):
    """[z >= 0] instead of [z > 0] on data with exact zeros and negative zeros, and a mask taken from a ROUNDED value
    (the product y * scale rounded to bf16 before the shift is added) instead of the fp32 pre-activation.  The mask of the
    stored activation, bf16(max(z, 0)) > 0, is the same mask -- bf16 has fp32's exponent range -- and must pass."""
    y, da, scale, shift = stream_case
    mean, istd = torch.zeros(8), torch.ones(8)
    bw = R.bn_relu_bwd(da, y, torch.bfloat16, scale, mean, istd, scale, shift)
    ge = R.bn_relu_bwd(da, y, torch.bfloat16, scale, mean, istd, scale, shift, mask_ge=True)
    assert bool((ge["on"] != bw["on"]).any())                     # the planted zeros are where the two masks differ
    with pytest.raises(AssertionError):
        R.assert_fp32(ge["dbeta"][0].float(), bw["dbeta"], "dbeta with >= mask")
    with pytest.raises(AssertionError):
        R.assert_bf16(_as_kernel_bf16(ge["dz"][0]), bw["dz"], "dz with >= mask")
    a = R.stored(R.bn_relu_apply(y, torch.bfloat16, scale, shift)[0], torch.bfloat16)
    assert torch.equal(a > 0, bw["on"])
    zr = R.stored(R.rd(y, torch.bfloat16) * scale.double()[None, :, None, None], torch.bfloat16) + shift.double()[None, :, None, None]
    assert bool(((zr > 0) != bw["on"]).any())
    with pytest.raises(AssertionError):
        R.assert_bf16(_as_kernel_bf16(R.rd(da, torch.bfloat16) * (zr > 0)), bw["dz"], "dz with the mask of a rounded product")


@pytest.mark.parametrize("offset", [1.0, 30.0])
def test_missing_and_repeated_row_group_is_rejected_at_the_largest_reduction(offset):
    """one 32-pixel row group missing from / counted twice in sum y, sum y^2 (seen through mean and E[y^2]), dbeta and dgamma
    at 2 097 152 pixels, with the smallest per-channel offset the large GPU cases use"""
    pixels = R.MAX_STREAM_PIXELS
    assert offset >= R.MIN_STREAM_OFFSET
    y = (_gen(60, (1, 2, pixels, 1)) + offset).bfloat16().double()
    da = (_gen(61, (1, 2, pixels, 1)) + offset).bfloat16().double()
    s = (y.sum((0, 2, 3)), y.abs().sum((0, 2, 3)))
    ss = ((y * y).sum((0, 2, 3)), (y * y).sum((0, 2, 3)))
    gamma, mean, istd = torch.ones(2), torch.zeros(2), torch.ones(2)          # yhat = y: dgamma = sum dz y
    bw = R.bn_relu_bwd(da, y, torch.bfloat16, gamma, mean, istd, torch.ones(2), torch.full((2,), 100.0))    # mask all on
    terms = {"sum y": (s, y), "sum y^2": (ss, y * y), "dbeta": (bw["dbeta"], da), "dgamma": (bw["dgamma"], da * y)}
    for name, (rs, t) in terms.items():
        R.assert_fp32(rs[0].float(), rs, "exact " + name)
        groups = t.view(2, -1, 32).sum(2)
        k = int(groups[0].abs().argsort()[groups.shape[1] // 2])            # a group of median weight
        for sign in (-1.0, 1.0):
            bad = rs[0].clone()
            bad[0] += sign * groups[0, k]
            with pytest.raises(AssertionError):
                R.assert_fp32(bad.float(), rs, f"{name} row group {'twice' if sign > 0 else 'missing'}")


def test_zero_mean_data_would_hide_a_missing_row_group():
    """why the large cases carry an offset: on zero-mean data the same defect is inside the bound"""
    y = _gen(62, (1, 1, R.MAX_STREAM_PIXELS, 1)).bfloat16().double()
    rs = (y.sum((0, 2, 3)), y.abs().sum((0, 2, 3)))
    groups = y.view(-1, 32).sum(1)
    bad = rs[0] - groups[int(groups.abs().argsort()[groups.numel() // 2])]
    assert R.assert_fp32(bad.float(), rs, "zero-mean, group missing") < 1.0


def test_wrong_variance_denominators_are_rejected():
    y, ga, be, rm, rv, _ = _bn_case(70, (2, 8, 12, 20))
    y = y.bfloat16().double()
    M = 2 * 12 * 20
    st = R.bn_train_stats(y, torch.bfloat16, ga, be, rm, rv, 0.1)
    var = st["var"][0]
    m = float(torch.tensor(0.1, dtype=torch.float32))
    with pytest.raises(AssertionError):           # running variance from the BIASED variance
        R.assert_fp32(((1 - m) * rv + m * var).float(), st["running_var"], "running var / count")
    with pytest.raises(AssertionError):           # normalisation with the UNBIASED variance
        R.assert_fp32((var * M / (M - 1) + EPS32).rsqrt().float(), st["istd"], "istd / (count - 1)")


def test_wrong_bilinear_weight_and_last_maximum_are_rejected():
    x = _gen(80, (1, 8, 16, 16))
    up = R.bilinear2x(x, torch.bfloat16)
    with pytest.raises(AssertionError):
        R.assert_bf16(_as_kernel_bf16(R.bilinear2x(x, torch.bfloat16, wrong=True)[0]), up, "H / 2H weights")
    a = _gen(81, (1, 8, 8, 8)).bfloat16().double()
    a[:, 0] = 0.5                                                      # a tie in every window of channel 0
    g = _gen(82, (1, 8, 4, 4)).bfloat16().double()
    good, bad = R.maxpool2_route(a, g), R.maxpool2_route(a, g, last=True)
    assert not torch.equal(good, bad) and torch.equal(good[:, 1:], bad[:, 1:])
    assert float(good[0, 0, 1::2].abs().max()) == 0 and float(good[0, 0, :, 1::2].abs().max()) == 0


@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_adam_defects_are_rejected_and_fp32_torch_is_accepted(decoupled):
    n = 4096 + 7
    p0, g = _gen(90, (n,)).float(), _gen(91, (n,)).float()
    m0, v0 = (_gen(92, (n,)) * 0.1).float(), (_gen(93, (n,)) ** 2 * 0.01).float()
    for step in (2, 1000):
        ref = R.adam_step(p0, g, m0, v0, step, weight_decay=1e-2, decoupled=decoupled)
        hp = torch.nn.Parameter(p0.clone())
        opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([hp], lr=1e-3, weight_decay=1e-2)
        opt.state[hp] = {"step": torch.tensor(float(step - 1)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
        hp.grad = g.clone()
        opt.step()
        host = hp.detach()
        R.assert_measured(host, ref[0], host, "fp32 torch against itself")
        assert R.MEASURED["fp32 torch against itself"][0] < 2.0 ** -22          # (so the floor is what binds on the host)
        if step == 2:
            late = R.adam_step(p0, g, m0, v0, step, weight_decay=1e-2, decoupled=decoupled, bias_step=step - 1)
            with pytest.raises(AssertionError):
                R.assert_measured(late[0][0].float(), ref[0], host, "bias correction of step t-1")
        other = R.adam_step(p0, g, m0, v0, step, weight_decay=1e-2, decoupled=decoupled, swap_decay=True)
        with pytest.raises(AssertionError):
            R.assert_measured(other[0][0].float(), ref[0], host, "the other decay rule")


# ---------------------------------------------------------------------- heads, MSE + focal loss, anomaly score
def test_head_and_loss_references_match_torch():
    from oracle import unet_oracle as O
    x, w, b = _gen(100, (2, 64, 5, 7)), _gen(101, (3, 64, 1, 1)) * 0.2, _gen(102, (3,))
    dout = _gen(103, (2, 3, 5, 7))
    for sigmoid in (False, True):
        xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        out = F.conv2d(xr, wr, br)
        out = torch.sigmoid(out) if sigmoid else out
        out.backward(dout)
        assert _close(R.head_fwd(x, F64, w, b, sigmoid)[0], out.detach())
        bw = R.head_bwd(x, F64, out.detach(), dout, w, sigmoid)
        assert _close(bw["dx"][0], xr.grad) and _close(bw["dw"][0], wr.grad) and _close(bw["db"][0], br.grad)
    recon, image = _gen(104, (2, 3, 6, 5)), _gen(105, (2, 3, 6, 5))
    amap = torch.rand(60, generator=torch.Generator().manual_seed(106), dtype=F64).view(2, 1, 6, 5)
    mask = (torch.rand(60, generator=torch.Generator().manual_seed(107)) < 0.3).double().view(2, 1, 6, 5)
    for gamma in (2.0, 1.5):
        rr, ar = recon.clone().requires_grad_(True), amap.clone().requires_grad_(True)
        bce = F.binary_cross_entropy(ar, mask, reduction="none")
        foc = (0.25 * (1 - torch.exp(-bce)) ** gamma * bce).mean()
        mse = F.mse_loss(rr, image)
        (foc + mse).backward()
        ref = R.mse_focal(recon, image, amap, mask, 0.25, gamma)
        assert _close(ref["mse"][0], mse.detach()) and _close(ref["focal"][0], foc.detach())
        assert _close(ref["d_recon"][0], rr.grad.reshape(-1)) and _close(ref["d_amap"][0], ar.grad.reshape(-1))
        d = O.combined_loss(recon, amap, image, mask, focal_gamma=gamma)           # the oracle is the same formula
        assert _close(ref["focal"][0], d["seg_loss"]) and _close(ref["mse"][0], d["recon_loss"])
    (sc, _), (im, _) = R.anomaly_score(recon, image)
    assert _close(sc, O.anomaly_score(recon, image)) and _close(im, O.anomaly_score(recon, image).flatten(1).mean(1))
    assert _close(R.anomaly_score(recon, image, l1=True)[0][0], (recon - image).abs().mean(1))


def test_head_exact_values_pass_and_truncated_or_short_sums_do_not():
    x, w, b = _gen(110, (2, 64, 24, 24)), (_gen(111, (8, 64, 1, 1)) * 0.2).float(), _gen(112, (8,)).float()
    z = R.head_fwd(x, torch.bfloat16, w, b, False)
    R.assert_fp32(z[0].float(), z, "exact logits")
    out = torch.sigmoid(z[0]).float()
    dout = _gen(113, (2, 8, 24, 24)).float()
    bw = R.head_bwd(x, torch.bfloat16, out, dout, w, True)
    R.assert_bf16(_as_kernel_bf16(bw["dx"][0]), bw["dx"], "exact head dx")
    R.assert_fp32(bw["dw"][0].float(), bw["dw"], "exact head dW")
    R.assert_fp32(bw["db"][0].float(), bw["db"], "exact head db")
    with pytest.raises(AssertionError):
        R.assert_bf16(R.round_bf16_toward_zero(bw["dx"][0]), bw["dx"], "truncated head dx")
    bad = z[0].clone()
    bad[0, 3, 5, 7] -= R.q64(x)[0, 17, 5, 7] * w.double()[3, 17, 0, 0]           # one of the 64 products missing
    with pytest.raises(AssertionError):
        R.assert_fp32(bad.float(), z, "logit with a dropped product")
    # the sigmoid is measured: fp32 torch passes against itself, a logit-level defect does not
    s = R.head_fwd(x, torch.bfloat16, w, b, True)
    host = torch.sigmoid(F.conv2d(R.q64(x).float(), w, b))
    R.assert_measured(host, s, host, "host sigmoid head", extra=R.SUM_EPS)
    with pytest.raises(AssertionError):
        R.assert_measured(torch.sigmoid(bad).float(), s, host, "sigmoid of the defective logit", extra=R.SUM_EPS)


def test_focal_edge_probabilities_are_finite_and_host_measured():
    from oracle import unet_oracle as O
    n = 4096
    amap = torch.rand(n, generator=torch.Generator().manual_seed(120))
    amap[:6] = torch.tensor([0.0, 1.0, 1e-30, 1 - 1e-7, 0.5, 1e-45])
    mask = (torch.rand(n, generator=torch.Generator().manual_seed(121)) < 0.1).float()
    recon, image = _gen(122, (n,)).float(), _gen(123, (n,)).float()
    ref = R.mse_focal(recon, image, amap, mask)
    assert all(bool(torch.isfinite(v[0]).all()) and bool(torch.isfinite(v[1]).all()) for v in ref.values())
    ar = amap.clone().requires_grad_(True)
    O.focal_loss(ar, mask).backward()
    R.assert_measured(ar.grad, ref["d_amap"], ar.grad, "host focal gradient")
    with pytest.raises(AssertionError):          # the gradient of gamma = 2 through the general pow path with gamma - 1 = 2
        R.assert_measured(R.mse_focal(recon, image, amap, mask, gamma=3.0)["d_amap"][0].float(), ref["d_amap"], ar.grad, "wrong gamma")


# ---------------------------------------------------------------------- fused head, SSIM
def test_fused_head_and_ssim_references_match_torch():
    from oracle import unet_oracle as O
    # fused head in float64 on fp32-exact operands (scale 1, shift 0, bf16-grid y): relu -> 1x1 conv -> sigmoid
    y = _gen(130, (2, 64, 5, 7)).bfloat16().double()
    w, b, dout = _gen(131, (3, 64, 1, 1)) * 0.2, _gen(132, (3,)), _gen(133, (2, 3, 5, 7))
    one, zero = torch.ones(64), torch.zeros(64)
    mean = _gen(134, (64,)).float()
    for sigmoid in (False, True):
        yr, wr, br = y.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        out = F.conv2d(F.relu(yr), wr, br)
        out = torch.sigmoid(out) if sigmoid else out
        out.backward(dout)
        assert _close(R.head_bnrelu_fwd(y, F64, one, zero, w, b, sigmoid)[0], out.detach())
        bw = R.head_bnrelu_bwd(y, F64, one, zero, mean, out.detach(), dout, w, sigmoid)
        assert _close(bw["dz"][0], yr.grad) and _close(bw["dw"][0], wr.grad) and _close(bw["db"][0], br.grad)
        assert torch.allclose(bw["sum"][0], yr.grad.sum((0, 2, 3)), rtol=1e-6, atol=1e-6)          # (over the fp32-STORED dz)
        assert torch.allclose(bw["sum_c"][0], (yr.grad * (y - mean.double()[None, :, None, None])).sum((0, 2, 3)), rtol=1e-6, atol=1e-5)
    a = torch.rand(2, 3, 20, 27, generator=torch.Generator().manual_seed(135), dtype=F64)
    c = _gen(136, (2, 3, 20, 27))
    for per_image in (False, True):
        ar, cr = a.clone().requires_grad_(True), c.clone().requires_grad_(True)
        v = O.ssim_loss(ar, cr, 11, size_average=not per_image)
        v.sum().backward()
        ref = R.ssim(a, c, 11, per_image)
        assert _close(ref["loss"][0], v.detach()) and _close(ref["d1"][0], ar.grad) and _close(ref["d2"][0], cr.grad)
        assert bool((ref["d1"][1] >= ref["d1"][0].abs() - 1e-15).all())


def test_ssim_host_passes_and_a_wrong_border_is_rejected():
    from oracle import unet_oracle as O
    a = torch.rand(1, 3, 40, 37, generator=torch.Generator().manual_seed(140))
    c = _gen(141, (1, 3, 40, 37)).float()
    ar, cr = a.clone().requires_grad_(True), c.clone().requires_grad_(True)
    v = O.ssim_loss(ar, cr)
    v.backward()
    ref = R.ssim(a, c)
    R.assert_measured(v.detach(), ref["loss"], v.detach(), "host ssim loss", extra=R.SUM_EPS)
    R.assert_measured(ar.grad, ref["d1"], ar.grad, "host ssim d1")
    # a blur that leaves out the last column of a frame that is not a multiple of the 32-pixel tile: replicate it by
    # taking the gradient of the frame cropped by one column
    bad = R.ssim(a[..., :36], c[..., :36])["d1"][0]
    with pytest.raises(AssertionError):
        R.assert_measured(bad.float(), (ref["d1"][0][..., :36], ref["d1"][1][..., :36]), ar.grad[..., :36], "cropped frame")
    fz = R.head_bnrelu_bwd(_gen(142, (1, 64, 4, 4)), torch.bfloat16, torch.ones(64), torch.zeros(64), torch.zeros(64),
                           torch.full((1, 2, 4, 4), 0.5), _gen(143, (1, 2, 4, 4)).float(), (_gen(144, (2, 64, 1, 1))).float(), True)
    R.assert_bf16(fz["dz_stored"].bfloat16(), fz["dz"], "exact fused dz")
    with pytest.raises(AssertionError):
        R.assert_bf16(R.round_bf16_toward_zero(fz["dz"][0]), fz["dz"], "truncated fused dz")


# ---------------------------------------------------------------------- segmentation loss (csrc/segloss.hip)
def _seg_case(seed, n, c, hw, ignore=255, frac_ignored=0.1, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    z = (scale * torch.randn((n, c, hw), generator=g)).float()
    t = torch.randint(0, c, (n, hw), generator=g)
    if frac_ignored:
        t[torch.rand((n, hw), generator=g) < frac_ignored] = ignore
    return z, t


def _torch_seg_loss(z, t, cw, ignore, ce_w, dice_w, focal_w, alpha, gamma):
    """the three terms with torch's own float64 operators and autograd"""
    zr = z.double().requires_grad_(True)
    n, c, hw = zr.shape
    valid = (t != ignore) & (t >= 0) & (t < c)
    ce = F.cross_entropy(zr, t, weight=None if cw is None else cw.double(), ignore_index=ignore)
    p = torch.softmax(zr, 1)
    onehot = torch.zeros_like(p).scatter_(1, torch.where(valid, t, torch.zeros_like(t))[:, None], valid[:, None].double())
    dice = 1 - ((2 * (p * onehot).sum(2) + 1e-8) / (p.sum(2) + onehot.sum(2) + 1e-8)).mean()
    nll = F.cross_entropy(zr, t, ignore_index=ignore, reduction="none")
    focal = (alpha * (1 - torch.exp(-nll)) ** gamma * nll).mean()
    total = ce_w * ce + dice_w * dice + focal_w * focal
    total.backward()
    return torch.stack([total, ce, dice, focal]).detach(), zr.grad


@pytest.mark.parametrize("c,gamma", [(4, 2.0), (3, 1.5), (8, 2.0), (1, 2.0)])
def test_seg_loss_reference_matches_torch_and_the_oracle(c, gamma):
    from oracle import seg_oracle as SO
    z, t = _seg_case(200 + c, 3, c, 157)
    t[1, :5] = -1                                            # (torch rejects these; the contract skips them like ignore_index)
    t[1, :5] = 255
    cw = torch.rand(c, generator=torch.Generator().manual_seed(7)).float() + 0.25
    alpha = float(torch.tensor(0.75, dtype=torch.float32))
    ref = R.seg_loss(z, t, cw, 255, 0.7, 1.3, 0.4, 0.75, gamma)
    want, grad = _torch_seg_loss(z, t, cw, 255, *(R._f32(v) for v in (0.7, 1.3, 0.4)), alpha, gamma)
    assert _close(ref["loss"][0], want) and _close(ref["dlogits"][0], grad)
    assert bool((ref["dlogits"][1] >= ref["dlogits"][0].abs() * (1 - 1e-12)).all())        # S bounds the value
    assert _close(ref["loss"][0][1], SO.cross_entropy(z, t, cw.double(), 255))
    if gamma == 2.0:
        assert _close(ref["loss"][0][3], SO.focal_loss(z, t, alpha, 2.0, 255))
    z2, t2 = _seg_case(210 + c, 2, c, 64, frac_ignored=0.0)
    r2 = R.seg_loss(z2, t2, None, -1, 1.0, 1.0, 0.0)
    assert _close(r2["loss"][0][2], SO.dice_loss(z2, t2)) and _close(r2["loss"][0][0], SO.combined_segmentation_loss(z2, t2))
    # a probability map: Dice on the map, the gradient with respect to the map
    pm = torch.softmax(z2, 1).float()
    pr = pm.double().requires_grad_(True)
    onehot = torch.zeros_like(pr).scatter_(1, t2[:, None], 1.0)
    d = 1 - ((2 * (pr * onehot).sum(2) + 1e-8) / (pr.sum(2) + onehot.sum(2) + 1e-8)).mean()
    d.backward()
    r3 = R.seg_loss(pm, t2, None, -1, 0.0, 1.0, 0.0, is_prob=True)
    assert _close(r3["loss"][0], torch.stack([d.detach(), d.detach()])) and _close(r3["dlogits"][0], pr.grad)


def test_seg_loss_contract_edges():
    """out-of-range labels are skipped like ignore_index, their probability stays in the Dice sum p; no valid pixel: CE 0
    with a zero CE gradient (torch: NaN); focal is a mean over all pixels"""
    z, t = _seg_case(220, 2, 3, 90)
    t2 = t.clone()
    t2[t == 255] = -3
    t3 = t.clone()
    t3[t == 255] = 3
    a, b, c = (R.seg_loss(z, x, None, 255, 1.0, 1.0, 1.0) for x in (t, t2, t3))
    assert torch.equal(a["loss"][0], b["loss"][0]) and torch.equal(a["dlogits"][0], c["dlogits"][0])
    none = R.seg_loss(z, torch.full_like(t, 255), None, 255, 1.0, 0.0, 0.0)
    assert float(none["loss"][0][1]) == 0.0 and float(none["dlogits"][0].abs().max()) == 0.0
    assert bool(torch.isnan(F.cross_entropy(z.double(), torch.full_like(t, 255), ignore_index=255)))
    dice_all_ignored = R.seg_loss(z, torch.full_like(t, 255), None, 255, 0.0, 1.0, 0.0)
    assert float(dice_all_ignored["loss"][0][2]) > 0.999999 and float(dice_all_ignored["dlogits"][0].abs().max()) > 0
    # the cross entropy follows the gap where -log of an fp32 probability sticks at 87.498 (and at 0 near pt = 1)
    for gap in (17.0, 20.0, 80.0, 87.0, 88.0, 100.0, 120.0):
        zz = torch.tensor([[[0.0], [-gap]]])
        wrong = R.seg_loss(zz, torch.tensor([[1]]), None, -1, 1.0, 0.0, 0.0, grad=False)
        right = R.seg_loss(zz, torch.tensor([[0]]), None, -1, 1.0, 0.0, 0.0, grad=False)
        lse = torch.log1p(torch.exp(torch.tensor(-gap, dtype=F64)))
        assert _close(wrong["loss"][0][1], gap + lse) and abs(float(right["loss"][0][1]) - float(lse)) < 1e-15


def _seg_emulation(z, t, cw, ignore, weights, defect=None, images=None):
    """what a correct (defect=None) or defective kernel stores: the float64 value rounded once to fp32"""
    r = R.seg_loss(z, t, cw, ignore, *weights, defect=defect, images=images)
    return r["loss"][0].float(), r["dlogits"][0].float()


def _rejects(ref, loss, grad, what):
    with pytest.raises(AssertionError):
        R.assert_seg(loss, grad, ref, what)


def test_seg_exact_and_host_values_are_accepted():
    z, t = _seg_case(230, 2, 4, 5000)
    z[0, :, :200] *= 12                                      # confident, and confidently wrong, pixels
    cw = torch.tensor([1.0, 50.0, 50.0, 0.0])
    ref = R.seg_loss(z, t, cw, 255, 1.0, 1.0, 0.5)
    w = R.assert_seg(ref["loss"][0].float(), ref["dlogits"][0].float(), ref, "exact")
    assert max(w.values()) < 0.5, w
    w = R.assert_seg(ref["loss_host"].float(), ref["dlogits_host"].float(), ref, "host")
    assert max(w.values()) <= 1.0, w
    assert R.MEASURED["host: dlogits"][2] < 2.0 ** -19       # the measured allowance stays at a few fp32 roundings of S
    pm = torch.softmax(z, 1)
    rp = R.seg_loss(pm, t, None, 255, 0.0, 1.0, 0.0, is_prob=True)
    R.assert_seg(torch.tensor([float(rp["loss"][0][0]), 0, float(rp["loss"][0][1]), 0]).float(), rp["dlogits"][0].float(), rp, "exact map")


@pytest.mark.parametrize("defect", ["b_sign", "a_class", "no_focal_dterm", "sump_skips_ignored", "focal_over_valid"])
def test_seg_formula_defects_are_rejected(defect):
    """at the Kolektor frame, 1024 x 512 with class weights 1 / 50 / 50 and about 1 % of the pixels in classes 1 and 2; the
    confident regime of the GPU tests (target margins 10 to 40) for the focal derivative term"""
    n, c, hw = 1, 3, 1024 * 512
    g = torch.Generator().manual_seed(240)
    z = (3 * torch.randn((n, c, hw), generator=g)).float()
    r = torch.rand((n, hw), generator=g)
    t = (r < 0.01).long() + (r < 0.005).long()
    t[torch.rand((n, hw), generator=g) < 0.1] = 255
    if defect == "no_focal_dterm":
        valid = t != 255
        margin = 10 + 30 * torch.rand((n, hw), generator=g)
        z.scatter_add_(1, torch.where(valid, t, torch.zeros_like(t))[:, None], (margin * valid)[:, None].float())
    cw = torch.tensor([1.0, 50.0, 50.0])
    weights = (1.0, 1.0, 0.5)
    ref = R.seg_loss(z, t, cw, 255, *weights)
    R.assert_seg(ref["loss"][0].float(), ref["dlogits"][0].float(), ref, "exact")
    loss, grad = _seg_emulation(z, t, cw, 255, weights, defect)
    if defect in ("b_sign", "a_class", "no_focal_dterm"):    # gradient-only defects
        assert torch.equal(loss, ref["loss"][0].float())
        _rejects(ref, ref["loss"][0].float(), grad, defect)
    else:                                                    # seen in the value and in the gradient, each on its own
        _rejects(ref, loss, None, defect)
        _rejects(ref, ref["loss"][0].float(), grad, defect)


@pytest.mark.parametrize("gap", [88.0, 100.0, 120.0])
def test_seg_clamped_cross_entropy_is_rejected(gap):
    """ce = -log(max(pt, 1e-38)) sticks at 87.498: one confidently wrong pixel in 4096 moves the CE, focal and total
    values.  The gradient only holds ce as pt ce, which is 0 there: a value defect, and the value comparison sees it."""
    z, t = _seg_case(250, 1, 3, 4096, frac_ignored=0.0)
    z[0, :, 7] = torch.tensor([0.0, -gap, -gap / 2])
    t[0, 7] = 1
    ref = R.seg_loss(z, t, None, -1, 1.0, 1.0, 0.5)
    loss, grad = _seg_emulation(z, t, None, -1, (1.0, 1.0, 0.5), "ce_clamp")
    for i, k in enumerate(R.SEG_OUTPUTS):
        one = ref["loss"][0].float()
        one[i] = loss[i]
        if k == "dice":
            assert one[i] == ref["loss"][0].float()[i]
        else:
            _rejects(ref, one, None, "clamped ce: " + k)
    R.assert_seg(ref["loss"][0].float(), grad, ref, "clamped ce: gradient")


def test_seg_missing_block_is_rejected_at_the_largest_image_and_batch():
    """one 4096-pixel block's partial missing from the sums of image 0: at the largest frame (per-image Dice sums) and in
    the largest batch (the CE denominator over N hw pixels), seen in the value and in image 0's gradient"""
    for n, c, hw, what in ((1, 2, R.MAX_SEG_IMAGE_HW, "image"), (48, 2, 512 * 512, "batch")):
        assert n * hw <= R.MAX_SEG_PIXELS and hw <= R.MAX_SEG_IMAGE_HW
        z, t = _seg_case(260 + n, n, c, hw, frac_ignored=0.05)
        for weights in ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0)) if what == "batch" else ((1.0, 1.0, 0.5),):
            ref = R.seg_loss(z, t, None, 255, *weights, images=[0])
            R.assert_seg(ref["loss"][0].float(), ref["dlogits"][0].float(), ref, "exact")
            loss, grad = _seg_emulation(z, t, None, 255, weights, "drop_block", images=[0])
            _rejects(ref, ref["loss"][0].float(), grad, f"missing block, {what}: gradient")
            if weights[1] > 0:                               # (a mean CE over 12 M pixels does not move: the gradient sees it)
                _rejects(ref, loss, None, f"missing block, {what}: value")


@pytest.mark.parametrize("c", [1, 2, 3, 4, 8])
def test_seg_missing_tail_pixel_is_rejected_up_to_the_sweep_limit(c):
    """the last pixel of image 0 missing from the sums, at the largest pixel count of the GPU sweep: the Dice coefficients
    of its class move by about 1 / hw, above the bound there -- and inside it at 1024 x 512, which is why the trainer
    shapes are not relied on for this defect"""
    hw = R.MAX_SEG_TAIL_HW_C1 if c == 1 else R.MAX_SEG_TAIL_HW
    z, t = _seg_case(270 + c, 2, c, hw, frac_ignored=0.1 if c == 1 else 0.0)
    t[0, -1] = 0
    ref = R.seg_loss(z, t, None, 255, 1.0, 1.0, 0.5)
    loss, grad = _seg_emulation(z, t, None, 255, (1.0, 1.0, 0.5), "drop_tail")
    if c == 1:               # one class: p = 1, the gradient is identically 0 and only the Dice value holds the sums,
        #                      2 v / (hw + v) with v valid pixels, which one pixel moves by 0.03 / hw at 10 % ignored
        assert float(ref["dlogits"][0].abs().max()) == 0.0
        _rejects(ref, loss, None, "missing tail pixel: value")
    else:
        _rejects(ref, ref["loss"][0].float(), grad, "missing tail pixel")
    if c == 3:
        z, t = _seg_case(279, 1, c, 1024 * 512, frac_ignored=0.0)
        ref = R.seg_loss(z, t, None, 255, 1.0, 1.0, 0.5)
        _, grad = _seg_emulation(z, t, None, 255, (1.0, 1.0, 0.5), "drop_tail")
        assert max(R.assert_seg(ref["loss"][0].float(), grad, ref, "tail pixel at 1024 x 512").values()) < 1.0


# ====================================================================== folded BatchNorm inference (conv3x3_bias_relu)
# An fp32-accumulating emulation of the kernel (bf16 operands, exact products, fp32 sums, fp32 shift, ReLU, one
# round-to-nearest-even store) passes; a shift from the wrong lane or channel tile, the ReLU on the wrong side of the
# shift or missing, the scale of the neighbouring row, a shift rounded to bf16 and a truncating store are rejected.
FOLD_SHAPES = [(2, 128, 128, 16, 32), (1, 512, 128, 16, 16), (1, 64, 192, 9, 21)]      # n, ci, co, h, w
FOLD_DEFECTS = ("shift_c4", "relu_first", "no_relu", "scale_row1", "shift_bf16", "truncate")


def _fold_case(shape):
    n, ci, co, h, w = shape
    seed = 1000 + ci + co + h
    x = _gen(seed, (n, ci, h, w)).float()
    wt = (_gen(seed + 1, (co, ci, 3, 3)) / (3 * ci ** 0.5)).float()
    rnd = torch.rand(2, co, generator=torch.Generator().manual_seed(seed + 2), dtype=F64)
    gamma, rv = (rnd[0] + 0.5).float(), (rnd[1] * 1.5 + 0.25).float()
    beta, rm = _gen(seed + 3, (co,)).float(), (_gen(seed + 4, (co,)) * 0.5).float()
    scale = gamma * (rv + 1e-5).rsqrt()                  # fp32, as read back from the coefficient kernel
    shift = beta - rm * scale                            # of the order of the activations (sigma ~ 1)
    return x, wt, scale, shift


def _fold_emulation(x, wt, scale, shift, defect=None):
    """the kernel in fp32 arithmetic on the CPU: bf16 operands, fp32 accumulation, shift and ReLU in fp32, one store"""
    sc = scale.roll(-1) if defect == "scale_row1" else scale
    wq = R.fold_weight(wt, sc).to(torch.bfloat16).float()
    acc = F.conv2d(x.to(torch.bfloat16).float(), wq, padding=1)
    sh = shift.roll(-4) if defect == "shift_c4" else shift.to(torch.bfloat16).float() if defect == "shift_bf16" else shift
    sh = sh[None, :, None, None]
    if defect == "relu_first":
        v = acc.clamp_min(0) + sh
    elif defect == "no_relu":
        v = acc + sh
    else:
        v = (acc + sh).clamp_min(0)
    return R.round_bf16_toward_zero(v) if defect == "truncate" else v.to(torch.bfloat16)


@pytest.fixture(scope="module", params=FOLD_SHAPES, ids=str)
def fold_case(request):
    x, wt, scale, shift = _fold_case(request.param)
    return x, wt, scale, shift, R.conv3x3_bias_relu(x, wt, scale, shift, torch.bfloat16)


def test_folded_conv_reference_matches_torch(fold_case):
    x, wt, scale, shift, (ref, S) = fold_case
    xq, wq = x.to(torch.bfloat16).double(), (wt * scale[:, None, None, None]).to(torch.bfloat16).double()
    assert _close(ref, torch.relu(F.conv2d(xq, wq, shift.double(), padding=1)))
    assert bool((S >= ref.abs()).all())
    lin = R.conv3x3_bias_relu(x, wt, scale, shift, torch.bfloat16, relu=False)[0]
    assert _close(lin.clamp_min(0), ref) and float(lin.min()) < 0
    # fp32 compute dtype: the folded weight is read unrounded
    r32 = R.conv3x3_bias_relu(x, wt, scale, shift, torch.float32)[0]
    assert _close(r32, torch.relu(F.conv2d(x.double(), (wt * scale[:, None, None, None]).double(), shift.double(), padding=1)))
    # the shift matters: of the order of the activations, distinct per channel
    assert float(shift.abs().mean()) > 0.3 and shift.unique().numel() == shift.numel()


def test_folded_conv_emulation_is_accepted(fold_case):
    x, wt, scale, shift, rs = fold_case
    worst = R.assert_bf16(_fold_emulation(x, wt, scale, shift), rs, "fp32-accumulating emulation")
    assert worst <= 1.0
    out32 = torch.relu(F.conv2d(x, R.fold_weight(wt, scale), shift, padding=1))
    R.assert_fp32(out32, R.conv3x3_bias_relu(x, wt, scale, shift, torch.float32), "fp32 emulation")


@pytest.mark.parametrize("defect", FOLD_DEFECTS)
def test_folded_conv_defects_are_rejected(fold_case, defect):
    x, wt, scale, shift, rs = fold_case
    with pytest.raises(AssertionError):
        R.assert_bf16(_fold_emulation(x, wt, scale, shift, defect), rs, defect)


# ====================================================================== fp32 compute dtype (test_gpu_staged.py)
# The fp32 kernels are held to 2^-18 S on UNROUNDED fp32 operands (dtype=torch.float32 of the references).  At the largest
# Ctot (256) and the largest weight-gradient K (5 x 17 x 35 = 2975 pixels) of the table of test_gpu_staged.py: the fp32
# host results pass, and operands narrowed to bf16 or to 10 explicit mantissa bits, one zeroed tap of one input channel,
# one 8 x 16 pixel tile missing from a weight-gradient reduction and an accumulate that drops the old value do not.
FP32_CONV_SHAPES = [(2, 128, 128, 20, 40), (1, 256, 192, 17, 35), (3, 128, 256, 7, 13), (1, 72, 64, 9, 21)]      # n, ci, co, h, w
FP32_WGRAD_SHAPES = [(2, 128, 128, 20, 40), (5, 256, 256, 17, 35)]          # K = 1600 and 2975 pixels
F32 = torch.float32


def _cut10(t):
    """fp32 cut to 10 explicit mantissa bits (the low 13 bits cleared)"""
    return (t.float().contiguous().view(torch.int32) & ~0x1FFF).view(torch.float32)


def _worst(fn, *a):
    """err / bound of a result that must be REJECTED, from the assertion's own text"""
    with pytest.raises(AssertionError) as e:
        fn(*a)
    return float(str(e.value).split(" = ")[1].split(" x bound")[0])


@pytest.fixture(scope="module", params=FP32_CONV_SHAPES, ids=str)
def fp32_conv(request):
    n, ci, co, h, w = request.param
    seed = 2000 + ci + co + h
    x, gy = _gen(seed, (n, ci, h, w)).float(), _gen(seed + 1, (n, co, h, w)).float()
    wt = (_gen(seed + 2, (co, ci, 3, 3)) / (3 * ci ** 0.5)).float()
    assert not torch.equal(x, x.bfloat16().float())               # the operands are NOT on the bf16 grid
    return x, wt, gy, R.conv3x3(x, wt, dtype=F32), R.conv3x3_dgrad(gy, wt, dtype=F32)


def test_fp32_references_read_unrounded_operands(fp32_conv):
    x, wt, gy, (ref, S), (dref, dS) = fp32_conv
    assert _close(ref, F.conv2d(x.double(), wt.double(), padding=1)) and bool((S >= ref.abs()).all())
    assert _close(dref, F.conv_transpose2d(gy.double(), wt.double(), padding=1))
    # the default stays the bf16 reference of every earlier caller
    assert torch.equal(R.conv3x3(x, wt)[0], F.conv2d(R.q64(x), R.q64(wt), padding=1))
    assert not _close(ref, R.conv3x3(x, wt)[0])


def test_fp32_host_convolution_is_accepted(fp32_conv):
    x, wt, gy, rs, drs = fp32_conv
    a = R.assert_fp32(F.conv2d(x, wt, padding=1), rs, "fp32 host conv")
    b = R.assert_fp32(F.conv_transpose2d(gy, wt, padding=1), drs, "fp32 host dgrad")
    print(f"\nREF64 staged cpu {tuple(x.shape)}: fp32 host conv {a:.3f} dgrad {b:.3f} of the bound")
    assert max(a, b) <= 1.0


@pytest.mark.parametrize("narrow", ["bf16", "10bit"])
def test_fp32_narrowed_operands_are_rejected(fp32_conv, narrow):
    x, wt, gy, rs, drs = fp32_conv
    cut = (lambda t: t.bfloat16().float()) if narrow == "bf16" else _cut10
    a = _worst(R.assert_fp32, F.conv2d(cut(x), cut(wt), padding=1), rs, f"{narrow} operands")
    b = _worst(R.assert_fp32, F.conv_transpose2d(cut(gy), cut(wt), padding=1), drs, f"{narrow} operands, dgrad")
    print(f"\nREF64 staged cpu {tuple(x.shape)}: {narrow} operands {a:.1f} dgrad {b:.1f} x bound")
    assert min(a, b) > 8.0                   # far outside, not at the edge (2^-9 and 2^-11 per operand against 2^-18)


def test_fp32_one_dropped_tap_is_rejected(fp32_conv):
    """one tap of one input channel zeroed for every output channel (a mis-zeroed halo piece / a skipped k step)"""
    x, wt, _, rs, _ = fp32_conv
    bad = wt.clone()
    bad[:, wt.shape[1] // 2, 0, 2] = 0
    assert _worst(R.assert_fp32, F.conv2d(x, bad, padding=1), rs, "dropped tap") > 100.0


def test_fp32_accumulate_that_drops_the_old_value_is_rejected(fp32_conv):
    x, wt, _, (ref, S), _ = fp32_conv
    old = _gen(2999, tuple(ref.shape)).float()
    acc = (ref + old.double(), S + old.double().abs())
    R.assert_fp32(old + F.conv2d(x, wt, padding=1), acc, "fp32 host accumulate")
    assert _worst(R.assert_fp32, F.conv2d(x, wt, padding=1), acc, "accumulate without the old value") > 100.0


@pytest.fixture(scope="module", params=FP32_WGRAD_SHAPES, ids=str)
def fp32_wgrad(request):
    n, ci, co, h, w = request.param
    seed = 3000 + ci + co + h
    x, gy = _gen(seed, (n, ci, h, w)).float(), _gen(seed + 1, (n, co, h, w)).float()
    return x, gy, R.conv3x3_wgrad(x, gy, dtype=F32)


def test_fp32_host_weight_gradient_is_accepted(fp32_wgrad):
    x, gy, rs = fp32_wgrad
    assert _close(rs[0], torch.nn.grad.conv2d_weight(x.double(), tuple(rs[0].shape), gy.double(), padding=1))
    got = R.assert_fp32(torch.nn.grad.conv2d_weight(x, tuple(rs[0].shape), gy, padding=1), rs, "fp32 host wgrad")
    print(f"\nREF64 staged cpu wgrad K {x.shape[0] * x.shape[2] * x.shape[3]}: fp32 host {got:.3f} of the bound")
    assert got <= 1.0


def test_fp32_missing_pixel_tile_of_a_weight_gradient_is_rejected(fp32_wgrad):
    """one 8 x 16 pixel tile of the last image (a split-K slab that was never written or never summed)"""
    x, gy, rs = fp32_wgrad
    cut = gy.clone()
    cut[-1, :, 8:16, 16:32] = 0
    bad = torch.nn.grad.conv2d_weight(x, tuple(rs[0].shape), cut, padding=1)
    assert _worst(R.assert_fp32, bad, rs, "missing tile") > 100.0
    assert float(((bad.double() - rs[0]).abs() > R.SUM_EPS * rs[1]).double().mean()) > 0.99      # every element sees it
    cutb = R.conv3x3_wgrad(x.bfloat16().float(), gy.bfloat16().float(), dtype=F32)[0].float()
    assert _worst(R.assert_fp32, cutb, rs, "bf16 operands, wgrad") > 8.0


def test_fp32_convt_references_read_unrounded_operands():
    x, w, b = _gen(3100, (2, 128, 5, 9)).float(), (_gen(3101, (128, 64, 2, 2)) * 0.1).float(), _gen(3102, (64,)).float()
    gy = _gen(3103, (2, 64, 10, 18)).float()
    y, dx = R.convt2x2(x, w, b, dtype=F32), R.convt2x2_dgrad(gy, w, dtype=F32)
    (dw, db) = R.convt2x2_wgrad(x, gy, dtype=F32)
    assert _close(y[0], F.conv_transpose2d(x.double(), w.double(), b.double(), stride=2))
    R.assert_fp32(F.conv_transpose2d(x, w, b, stride=2), y, "fp32 host convT")
    R.assert_fp32(F.conv2d(gy, w, stride=2), dx, "fp32 host convT dgrad")
    R.assert_fp32(torch.einsum("nihw,nohywx->ioyx", x, gy.view(2, 64, 5, 2, 9, 2)), dw, "fp32 host convT wgrad")
    R.assert_fp32(gy.sum((0, 2, 3)), db, "fp32 host convT bias gradient")
    assert _worst(R.assert_fp32, F.conv_transpose2d(x.bfloat16().float(), w.bfloat16().float(), b, stride=2), y, "bf16") > 8.0
    assert _worst(R.assert_fp32, F.conv2d(gy.bfloat16().float(), w.bfloat16().float(), stride=2), dx, "bf16 dgrad") > 8.0
