"""CPU self-test of tests/_ref64.py: the exact reference passes its own comparator, and the defects the bf16 GPU tests
are there to catch -- one dropped product term, truncating instead of round-to-nearest-even, one missing 32-pixel
block of a weight-gradient reduction at the largest K the suite uses -- are rejected."""
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
