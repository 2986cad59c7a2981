"""The BatchNorm-backward tails whose masked gradient dz comes from a cheap streaming producer -- the 1x1 head over a
conv-BatchNorm-ReLU layer and the pooled encoder layers -- write dy once: a pass that only sums
(unet_head_bnrelu_bwd_sums / unet_bn_relu_pool_bwd_sums), the coefficient-only unet_bn_bwd_premasked(dy = NULL), and a
pass that forms dz again and writes dy = A*dz + B*y + K (unet_head_bnrelu_bwd_apply / unet_bn_relu_pool_bwd_apply).

The split repeats the arithmetic of the two-pass pair (unet_head_bnrelu_bwd or unet_bn_relu_pool_bwd, then
unet_bn_bwd_premasked in place), so every output is compared with torch.equal: dy, dgamma, dbeta, the head's dW / db,
the partial rows and the coefficients.  No tolerance applies.

Shapes are the smallest that reach every path: frames that are and are not a multiple of the 64-pixel wave tile, more
than one block, head widths 1 and 3 (the tile kernel at 64 channels, the generic one at 32 and 128), whole and ragged
pool windows, the skip gradient absent, present and overwritten in place."""
import ctypes as C

import pytest
import torch

from oracle import weights as W

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]


@pytest.fixture(scope="module")
def hip():
    from tiaozhanbei_unet_amd import _lib, ops
    return _lib, ops


def dev():
    return torch.device("cuda:0")


def rnd(name, shape):
    return W.make_input("tail:" + name, shape)


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def nhwc(t, dtype):
    return t.to(dev()).to(dtype).contiguous(memory_format=torch.channels_last)


def _layer(tag, n, c, h, w, dtype, mask):
    """Raw conv output y (NHWC, compute dtype) with per-channel offsets and the layer's BatchNorm values
    coef = [mean, istd, scale, shift] on the device.  mask: "half" -- batch statistics, so about half of
    z = y*scale + shift is positive; "all" / "none" -- every element masked / none."""
    y = rnd(tag + "_y", (n, c, h, w)) * 1.5 + rnd(tag + "_off", (c,))[None, :, None, None] * 2.0
    gamma, beta = rnd(tag + "_g", (c,)) * 0.5 + 1.0, rnd(tag + "_b", (c,)) * 0.2
    yq = y.to(dtype).double()
    mean = yq.mean((0, 2, 3))
    istd = (yq.var((0, 2, 3), unbiased=False) + 1e-5).rsqrt()
    scale = gamma.double() * istd
    shift = beta.double() - mean * scale
    if mask != "half":
        scale = torch.zeros_like(scale)
        shift = torch.full_like(shift, -1.0 if mask == "all" else 1.0)
    coef = torch.stack([mean, istd, scale, shift]).float().to(dev())
    return nhwc(y, dtype), gamma.to(dev()), coef


def _premasked(L, dt, dz, y, pixels, c, gamma, coef, part, nparts):
    """unet_bn_bwd_premasked; dz given: the apply pass in place, dz None: coefficients only.  -> dgamma, dbeta, A/B/K"""
    dgam, dbet = torch.empty(c, device=dev()), torch.empty(c, device=dev())
    cf = torch.empty(3 * c, device=dev())
    L.check(L.lib().unet_bn_bwd_premasked(dt, p(dz), None if dz is None else p(y), pixels, c, p(gamma), p(coef[0]), p(coef[1]),
                                          p(part), nparts, p(dgam), p(dbet), p(dz), p(cf), cf.numel() * 4, st()),
            "unet_bn_bwd_premasked")
    return dgam, dbet, cf


def _same(new, old, what):
    assert new.dtype == old.dtype and new.shape == old.shape, what
    assert torch.equal(new, old), f"{what}: {int((new != old).sum())} of {new.numel()} elements differ"


# ------------------------------------------------------------------------------------------------------------ head
HEAD_CASES = [(ci, frame, co, sig, "half") for ci in (64,) for frame in ((16, 16), (20, 12)) for co in (1, 3)
              for sig in (True, False)]
HEAD_CASES += [(64, (20, 12), 3, True, "all"), (64, (20, 12), 1, True, "none")]
# the generic kernel (channel counts other than 64), several blocks with a ragged last tile (64 x 36 x 2 = 4608 pixels + ...)
HEAD_CASES += [(128, (20, 12), 3, True, "half"), (32, (20, 12), 1, False, "half"), (64, (50, 47), 3, True, "half")]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("ci,frame,co,sigmoid,mask", HEAD_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_head_tail_writes_dy_once(hip, dtype, ci, frame, co, sigmoid, mask):
    L, ops = hip
    lib = L.lib()
    n, (h, w) = 2, frame
    dt = ops._DT[dtype]
    tag = f"h{ci}_{h}x{w}_{co}"
    yd, gamma, coef = _layer(tag, n, ci, h, w, dtype, mask)
    wd = (rnd(tag + "_w", (co, ci, 1, 1)) * 0.2).to(dev()).contiguous()
    bd = (rnd(tag + "_bias", (co,)) * 0.1).to(dev())
    dout = rnd(tag + "_dout", (n, co, h, w)).to(dev()).contiguous()
    out = torch.empty(n, co, h, w, device=dev())
    L.check(lib.unet_head_bnrelu_fwd(dt, p(yd), n, h, w, ci, p(coef[2]), p(coef[3]), p(wd), p(bd), co, int(sigmoid), p(out),
                                     st()), "unet_head_bnrelu_fwd")
    cap, need = lib.unet_head_bnrelu_max_parts(), lib.unet_head_bwd_workspace(n, h, w, ci, co)

    def phase1(fn, dz):
        dwh, dbh = torch.empty(co, ci, 1, 1, device=dev()), torch.empty(co, device=dev())
        part, nparts = torch.zeros(cap, 2, ci, device=dev()), C.c_int32(0)
        ws = torch.empty(need, dtype=torch.uint8, device=dev())
        args = [dt, p(yd), p(coef[2]), p(coef[3]), p(coef[0]), p(out), p(dout), n, h, w, ci, p(wd), co, int(sigmoid)]
        args += ([p(dz)] if dz is not None else []) + [p(dwh), p(dbh), p(part), C.byref(nparts), p(ws), need, st()]
        L.check(fn(*args), "head backward, phase 1")
        assert 0 < nparts.value <= cap
        return dwh, dbh, part, nparts.value

    dy_old = ops._nhwc_empty(n, ci, h, w, dtype, dev())
    dw_old, db_old, part_old, np_old = phase1(lib.unet_head_bnrelu_bwd, dy_old)
    masked = float((dy_old == 0).float().mean())
    assert {"half": 0.25 < masked < 0.75, "all": masked == 1.0, "none": masked < 0.01}[mask], masked
    dg_old, dbeta_old, cf_old = _premasked(L, dt, dy_old, yd, n * h * w, ci, gamma, coef, part_old, np_old)

    dw_new, db_new, part_new, np_new = phase1(lib.unet_head_bnrelu_bwd_sums, None)
    dg_new, dbeta_new, cf_new = _premasked(L, dt, None, None, n * h * w, ci, gamma, coef, part_new, np_new)
    dy_new = ops._nhwc_empty(n, ci, h, w, dtype, dev())
    L.check(lib.unet_head_bnrelu_bwd_apply(dt, p(yd), p(coef[2]), p(coef[3]), p(out), p(dout), n, h, w, ci, p(wd), co,
                                           int(sigmoid), p(cf_new), p(dy_new), st()), "unet_head_bnrelu_bwd_apply")
    torch.cuda.synchronize()
    assert np_new == np_old
    _same(part_new[:np_new], part_old[:np_old], "partial rows")
    _same(dw_new, dw_old, "head dW")
    _same(db_new, db_old, "head db")
    _same(dg_new, dg_old, "dgamma")
    _same(dbeta_new, dbeta_old, "dbeta")
    _same(cf_new, cf_old, "A, B, K")
    _same(dy_new, dy_old, "dy")


# ------------------------------------------------------------------------------------------------------------ pool
# 16x16 / 12x20 / 18x14: whole windows (18x14 pools to the odd 9x7); 15x13: ragged last row and column of windows
POOL_CASES = [(c, frame, skip, "half") for c in (64, 128) for frame in ((16, 16), (12, 20), (18, 14), (15, 13))
              for skip in ("none", "given", "inplace")]
POOL_CASES += [(64, (18, 14), "inplace", "all"), (64, (18, 14), "inplace", "none")]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("c,frame,skip,mask", POOL_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_pool_tail_writes_dy_once(hip, dtype, c, frame, skip, mask):
    L, ops = hip
    lib = L.lib()
    n, (h, w) = 2, frame
    dt = ops._DT[dtype]
    tag = f"p{c}_{h}x{w}"
    yd, gamma, coef = _layer(tag, n, c, h, w, dtype, mask)
    dpooled = nhwc(rnd(tag + "_dp", (n, c, h // 2, w // 2)), dtype)
    da = None if skip == "none" else nhwc(rnd(tag + "_da", (n, c, h, w)), dtype)
    cap = lib.unet_bn_relu_pool_max_parts()

    def buffers():
        """(skip gradient the kernels read, destination): the same tensor when the skip's buffer is overwritten"""
        src = None if da is None else da.clone(memory_format=torch.preserve_format)
        return src, (src if skip == "inplace" else ops._nhwc_empty(n, c, h, w, dtype, dev()))

    src, dy_old = buffers()
    part_old, nparts = torch.zeros(cap, 2, c, device=dev()), C.c_int32(0)
    L.check(lib.unet_bn_relu_pool_bwd(dt, p(yd), p(dpooled), p(src), n, h, w, c, p(coef[2]), p(coef[3]), p(coef[0]), p(dy_old),
                                      p(part_old), C.byref(nparts), st()), "unet_bn_relu_pool_bwd")
    np_old = nparts.value
    assert 0 < np_old <= cap
    masked = float((dy_old == 0).float().mean())
    assert {"half": 0.25 < masked < 0.9, "all": masked == 1.0, "none": masked < 0.8}[mask], masked
    dg_old, dbeta_old, cf_old = _premasked(L, dt, dy_old, yd, n * h * w, c, gamma, coef, part_old, np_old)

    src, dy_new = buffers()
    part_new, nparts = torch.zeros(cap, 2, c, device=dev()), C.c_int32(0)
    L.check(lib.unet_bn_relu_pool_bwd_sums(dt, p(yd), p(dpooled), p(src), n, h, w, c, p(coef[2]), p(coef[3]), p(coef[0]),
                                           p(part_new), C.byref(nparts), st()), "unet_bn_relu_pool_bwd_sums")
    np_new = nparts.value
    if src is not None:
        _same(src, da, "the skip gradient after the summing pass")
    dg_new, dbeta_new, cf_new = _premasked(L, dt, None, None, n * h * w, c, gamma, coef, part_new, np_new)
    L.check(lib.unet_bn_relu_pool_bwd_apply(dt, p(yd), p(dpooled), p(src), n, h, w, c, p(coef[2]), p(coef[3]), p(cf_new),
                                            p(dy_new), st()), "unet_bn_relu_pool_bwd_apply")
    torch.cuda.synchronize()
    assert np_new == np_old
    _same(part_new[:np_new], part_old[:np_old], "partial rows")
    _same(dg_new, dg_old, "dgamma")
    _same(dbeta_new, dbeta_old, "dbeta")
    _same(cf_new, cf_old, "A, B, K")
    _same(dy_new, dy_old, "dy")
    if skip == "given":
        _same(src, da, "a skip gradient that is not ours to overwrite")
