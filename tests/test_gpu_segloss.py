"""unet_seg_loss (csrc/segloss.hip) through the C ABI against the float64 reference _ref64.seg_loss, at the pixel counts
where the block partition changes, at the trainers' frame sizes and in the logit regimes where an fp32 softmax loses
its footing.

seg_reduce_kernel gives an image bpi = min(cdiv(hw, 4096), 2048 / n) blocks of per = cdiv(hw, bpi) pixels (restated in
plan() below); seg_finalize_kernel adds the n * bpi partials in a fixed order in fp64; seg_grad_kernel runs
min(cdiv(hw, 1024), 1024) blocks per image and strides above 1 048 576 pixels.  (bpi * per >= hw with
(bpi - 1) * per < hw for every n and hw the launcher accepts: a block may be short, never empty.)

Every case holds the four loss values and EVERY gradient element to the derived bounds of _ref64.seg_loss (no tie
region, nothing left out), with sentinel margins around loss, dlogits and the workspace.  The worst err / bound per
output is printed as 'REF64 segloss ...' lines.

The confidently-wrong cases (target logit 80 ... 120 below the maximum) need the cross entropy formed from the
log-sum-exp: -log(max(pt, 1e-38)) of the normalised probability sticks at 87.498 from a gap of about 87.3 on.
"""
import ctypes as C

import pytest
import torch

import _ref64 as R
from tiaozhanbei_unet_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 4096          # sentinel bytes before and after every guarded buffer
SENTINEL = 0xA5
NSUM = 27              # floats per block partial: I[8], P[8], T[8], ce numerator, ce denominator, focal
GAPS = (80.0, 87.0, 88.0, 100.0, 120.0)
SWEEP_HW = (1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8193, 12289)
REGIMES = ("normal", "confident", "wrong", "ties", "equal")
TARGETS = ("plain", "absent", "ignored", "all_ignored", "zero_weight", "ignore_in_range")


def cdiv(a, b):
    return -(-a // b)


def plan(n, hw):
    """(bpi, per, pixels of the last block, blocks of seg_grad_kernel): the launcher's integer formulas"""
    bpi = max(1, min(cdiv(hw, 4096), max(2048 // n, 1)))
    per = cdiv(hw, bpi)
    return bpi, per, hw - (bpi - 1) * per, min(cdiv(hw, 1024), 1024)


def _guarded(nbytes):
    buf = torch.full((nbytes + 2 * MARGIN,), SENTINEL, dtype=torch.uint8, device=DEV)
    return buf, buf.data_ptr() + MARGIN


def _intact(buf):
    return bool((buf[:MARGIN] == SENTINEL).all()) and bool((buf[-MARGIN:] == SENTINEL).all())


def call(z, t, cw=None, ignore=-1, weights=(1.0, 1.0, 0.0), alpha=1.0, gamma=2.0, is_prob=False, grad=True,
         ws_bytes=None, c_arg=None):
    """-> (status, loss[4] cpu, dlogits cpu or None, the guarded buffers).  z [n, c, hw] fp32, t [n, hw] int64 (host)."""
    n, c, hw = z.shape
    c_arg = c if c_arg is None else c_arg
    lib = L.lib()
    need = lib.unet_seg_loss_workspace(n, c_arg, hw)
    bpi = plan(n, hw)[0]
    assert need == (n * bpi * NSUM + 6 + 2 * n * c_arg) * 4, "workspace size is not the documented partition"
    zd, td = z.to(DEV).contiguous(), t.to(DEV).contiguous()
    cwd = None if cw is None else cw.to(DEV).float().contiguous()
    assert zd.numel() == n * c * hw and td.numel() == n * hw and (cwd is None or cwd.numel() >= c)
    bufs = {"loss": _guarded(16), "ws": _guarded(need)}
    if grad:
        bufs["dlogits"] = _guarded(zd.numel() * 4)
    rc = lib.unet_seg_loss(C.c_void_p(zd.data_ptr()), C.c_void_p(td.data_ptr()), n, c_arg, hw,
                           None if cwd is None else C.c_void_p(cwd.data_ptr()), ignore, 1 if is_prob else 0, *weights, alpha,
                           gamma, C.c_void_p(bufs["loss"][1]), C.c_void_p(bufs["dlogits"][1]) if grad else None,
                           C.c_void_p(bufs["ws"][1]), need if ws_bytes is None else ws_bytes, None)
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        assert _intact(buf), f"{k}: a store landed outside the buffer"
    loss = bufs["loss"][0][MARGIN:-MARGIN].view(torch.float32).cpu()
    dl = bufs["dlogits"][0][MARGIN:-MARGIN].view(torch.float32).cpu().view(n, c, hw) if grad else None
    return rc, loss, dl, bufs


def make_logits(regime, n, c, hw, t, seed):
    g = torch.Generator().manual_seed(seed)
    z = (3 * torch.randn((n, c, hw), generator=g)).float()         # the fixtures' 3 N(0, 1)
    valid = (t >= 0) & (t < c)
    tc = torch.where(valid, t, torch.zeros_like(t))[:, None]
    if regime == "confident":                                      # target margins 10 ... 40: pt within an ulp of 1
        margin = 10 + 30 * torch.rand((n, hw), generator=g)
        z = (z / 3).scatter_add(1, tc, (margin * valid)[:, None].float())
    elif regime == "wrong":                                        # every 7th pixel: the target sits `gap` below the maximum
        gap = torch.tensor(GAPS)[torch.arange(hw) % len(GAPS)].expand(n, hw)
        low = (z.max(1).values - gap)[:, None]
        pick = (valid & (torch.arange(hw) % 7 == 0).expand(n, hw))[:, None]
        z = torch.where(pick & (torch.arange(c)[None, :, None] == tc), low, z)
    elif regime == "ties":                                         # few levels: exact ties, the maximum included
        z = torch.randn((n, c, hw), generator=g).round().float()
    elif regime == "equal":
        z = torch.full((n, c, hw), 0.5)
    return z.float().contiguous()


def make_target(mode, n, c, hw, seed):
    """-> (labels, ignore_index, class weights)"""
    g = torch.Generator().manual_seed(seed + 1)
    t = torch.randint(0, c, (n, hw), generator=g)
    cw = (torch.rand(c, generator=g) + 0.5).float()
    ignore = 255
    if mode == "absent":                                           # class c - 1 nowhere, class 0 not in image 0, the last
        t = torch.randint(0, max(c - 1, 1), (n, hw), generator=g)  # image of a batch holds a single class
        if c > 1:
            t[0][t[0] == 0] = min(1, c - 1)
        if n > 1:
            t[-1] = min(1, c - 1)
    elif mode == "ignored":                                        # a fraction ignored, negative and >= c labels, and one
        r = torch.rand((n, hw), generator=g)                       # image of a batch ignored altogether
        t[r < 0.1] = ignore
        t[(r >= 0.1) & (r < 0.13)] = -1
        t[(r >= 0.13) & (r < 0.16)] = c
        t[(r >= 0.16) & (r < 0.17)] = -(2 ** 40)
        if n > 1:
            t[1] = ignore
    elif mode == "all_ignored":
        t[:] = ignore
    elif mode == "zero_weight":
        cw[c - 1] = 0.0
    elif mode == "ignore_in_range":
        ignore = c - 1
    elif mode == "rare":                                           # about 1 % of the pixels in classes 1 and 2
        r = torch.rand((n, hw), generator=g)
        t = (r < 0.01).long() + (r < 0.005).long()
        cw = torch.tensor([1.0, 50.0, 50.0] + [1.0] * (c - 3))[:c]
    return t, ignore, cw


def check(what, z, t, cw, ignore, weights, alpha=1.0, gamma=2.0, grad=True):
    rc, loss, dl, _ = call(z, t, cw, ignore, weights, alpha, gamma, grad=grad)
    assert rc == 0, (what, L.lib().unet_last_error())
    ref = R.seg_loss(z, t, cw, ignore, *weights, alpha, gamma, grad=grad)
    worst = R.assert_seg(loss, dl, ref, what)
    print(f"\nREF64 segloss {what}: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()), flush=True)
    return worst, loss, dl, ref


def test_plan_reaches_every_partition_branch():
    """the cases reach one block, a second block one pixel short of the first, uneven per with a short last block, the
    2048 / n cap and the grad stride"""
    assert plan(1, 4096)[:3] == (1, 4096, 4096) and plan(1, 4097)[:3] == (2, 2049, 2048)
    assert plan(1, 8193)[:3] == (3, 2731, 2731) and plan(3, 12289)[:3] == (4, 3073, 3070)
    assert plan(48, 512 * 512)[:3] == (42, 6242, 6222) and cdiv(512 * 512, 4096) > 2048 // 48
    assert plan(1, 1408 * 1024)[3] == 1024 and 1408 * 1024 > 1024 * 1024          # seg_grad_kernel strides
    assert plan(2, 1024 * 512)[3] == 512
    for n in (1, 2, 3, 48, 512):
        for hw in SWEEP_HW + (512 * 512, 1024 * 512, 1408 * 1024):
            bpi, per, last, _ = plan(n, hw)
            assert 0 < last <= per, (n, hw)
    # a missing tail pixel is only relied on within these (test_cpu_ref64.py plants it there); one class: the small counts
    assert max(SWEEP_HW) <= R.MAX_SEG_TAIL_HW and sum(hw <= R.MAX_SEG_TAIL_HW_C1 for hw in SWEEP_HW) >= 7


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("c", [1, 2, 3, 4, 8])
def test_pixel_count_sweep(c, n):
    """every partition edge x class count, all three terms on, class weights, a tenth of the pixels not valid"""
    for i, hw in enumerate(SWEEP_HW):
        t, ignore, cw = make_target("ignored" if hw > 65 else "plain", n, c, hw, 1000 * c + hw)
        z = make_logits(REGIMES[i % 3], t.shape[0], c, hw, t, 77 * c + hw + n)
        check(f"sweep c={c} n={t.shape[0]} hw={hw} {REGIMES[i % 3]}", z, t, cw, ignore, (1.0, 1.0, 0.5), 0.75)


@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("regime", REGIMES)
def test_logit_regimes_and_targets(regime, target):
    for c, n, hw in ((3, 2, 4097), (8, 3, 12289)):
        t, ignore, cw = make_target(target, n, c, hw, 31 * c + hw)
        z = make_logits(regime, n, c, hw, t, 5 * c + hw)
        worst, loss, dl, ref = check(f"{regime} {target} c={c} n={n} hw={hw}", z, t, cw, ignore, (1.0, 1.0, 0.5))
        if target == "all_ignored":          # pinned: CE is 0 with a zero CE gradient where torch gives NaN
            assert float(loss[1]) == 0.0 and float(loss[3]) == 0.0
            rc, l2, d2, _ = call(z, t, cw, ignore, (1.0, 0.0, 1.0))
            assert rc == 0 and float(l2[0]) == 0.0 and float(d2.abs().max()) == 0.0
        if regime == "equal" and target == "plain":
            assert abs(float(loss[1]) - torch.log(torch.tensor(float(c))).item()) < 1e-6


@pytest.mark.parametrize("gap", GAPS)
def test_cross_entropy_follows_any_gap(gap):
    """every pixel confidently wrong by the same gap: CE = gap + log(sum), focal alike, to the float64 value"""
    c, n, hw = 3, 1, 4097
    t = torch.randint(0, c, (n, hw), generator=torch.Generator().manual_seed(int(gap)))
    z = torch.zeros((n, c, hw)).scatter_(1, t[:, None], torch.full((n, 1, hw), -gap))
    worst, loss, _, ref = check(f"gap {gap:g}", z, t, None, -1, (1.0, 1.0, 1.0))
    want = gap + torch.log(torch.tensor(2.0, dtype=torch.float64) + torch.exp(torch.tensor(-gap, dtype=torch.float64)))
    assert abs(float(ref["loss"][0][1]) - float(want)) < 1e-12


TRAINER = [
    # what, n, c, hw, target mode, regimes
    ("kolektor 1024x512", 2, 3, 1024 * 512, "rare", ("normal", "confident", "wrong")),
    ("gear 512x512", 2, 8, 512 * 512, "ignored", ("normal", "confident")),
    ("1408x512", 1, 4, 1408 * 512, "plain", ("normal",)),
    ("1408x1024 (grad stride)", 1, 2, 1408 * 1024, "ignored", ("normal", "wrong")),
    ("batch 48 x 512x512 (block cap)", 48, 2, 512 * 512, "ignored", ("normal",)),
]


@pytest.mark.parametrize("case", TRAINER, ids=[c[0].split(" (")[0].replace(" ", "-") for c in TRAINER])
def test_trainer_shapes(case):
    what, n, c, hw, target, regimes = case
    assert hw <= R.MAX_SEG_IMAGE_HW and n * hw <= R.MAX_SEG_PIXELS
    t, ignore, cw = make_target(target, n, c, hw, 17 * c + n)
    for regime in regimes:
        z = make_logits(regime, n, c, hw, t, 3 * c + n)
        check(f"{what} c={c} n={n} {regime}", z, t, cw, ignore, (1.0, 1.0, 0.5))


@pytest.mark.parametrize("weights,gamma", [((1.0, 0.0, 0.0), 2.0), ((0.0, 1.0, 0.0), 2.0), ((0.0, 0.0, 1.0), 2.0),
                                           ((0.7, 1.3, 0.4), 2.0), ((1.0, 1.0, 1.0), 1.5), ((0.0, 0.0, 1.0), 3.0)])
def test_term_switches_and_value_only(weights, gamma):
    c, n, hw = 4, 2, 8193
    t, ignore, cw = make_target("ignored", n, c, hw, 9)
    for regime in ("normal", "confident"):
        z = make_logits(regime, n, c, hw, t, 11)
        _, loss, dl, _ = check(f"terms {weights} gamma={gamma} {regime}", z, t, cw, ignore, weights, 0.25, gamma)
        _, only, none, _ = check(f"terms {weights} gamma={gamma} {regime} value-only", z, t, cw, ignore, weights, 0.25, gamma,
                                 grad=False)
        assert none is None and torch.equal(only, loss)


def test_probability_map_dice():
    for c, n, hw in ((4, 2, 8193), (8, 1, 512 * 512), (1, 2, 257)):
        t, ignore, _ = make_target("ignored", n, c, hw, 21)
        pm = torch.softmax(make_logits("normal", n, c, hw, t, 22), 1).contiguous()
        if c == 1:
            pm = torch.rand((n, c, hw), generator=torch.Generator().manual_seed(23))
        rc, loss, dl, _ = call(pm, t, None, ignore, (0.0, 1.0, 0.0), is_prob=True)
        assert rc == 0
        ref = R.seg_loss(pm, t, None, ignore, 0.0, 1.0, 0.0, is_prob=True)
        worst = R.assert_seg(loss, dl, ref, f"probability map c={c}")
        print(f"\nREF64 segloss probability map c={c} n={n} hw={hw}: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()), flush=True)


def test_two_runs_are_bitwise_equal():
    for c, n, hw in ((3, 2, 1024 * 512), (8, 3, 12289)):
        t, ignore, cw = make_target("ignored", n, c, hw, 41)
        z = make_logits("normal", n, c, hw, t, 42)
        a, b = (call(z, t, cw, ignore, (1.0, 1.0, 0.5)) for _ in range(2))
        assert a[0] == 0 and b[0] == 0
        assert a[1].numpy().tobytes() == b[1].numpy().tobytes() and a[2].numpy().tobytes() == b[2].numpy().tobytes()


def test_refusals_leave_every_buffer_untouched():
    lib = L.lib()
    t = torch.zeros((2, 300), dtype=torch.int64)
    z9 = torch.zeros((2, 9, 300))
    need = lib.unet_seg_loss_workspace(2, 4, 300)
    for what, kw, z in (("c = 9", dict(c_arg=9), z9), ("short workspace", dict(ws_bytes=need - 1), z9[:, :4].contiguous()),
                        ("map with CE", dict(is_prob=True, weights=(1.0, 1.0, 0.0)), z9[:, :4].contiguous()),
                        ("map with focal", dict(is_prob=True, weights=(0.0, 1.0, 0.5)), z9[:, :4].contiguous())):
        rc, _, _, bufs = call(z, t, **kw)                           # (call() asserts the margins)
        assert rc != 0, what
        assert len(lib.unet_last_error()) > 0
        for k, (buf, _) in bufs.items():
            assert bool((buf == SENTINEL).all()), f"{what}: {k} was written"


def test_python_loss_scales_the_c_abi_gradient():
    from tiaozhanbei_unet_amd import metrics as M
    c, n, h, w = 3, 2, 40, 52
    t, ignore, cw = make_target("ignored", n, c, h * w, 51)
    z = make_logits("normal", n, c, h * w, t, 52).bfloat16().float()              # bf16-exact logits
    rc, loss, dl, _ = call(z, t, cw, ignore, (1.0, 1.0, 0.5))
    assert rc == 0
    crit = M.CombinedSegmentationLoss(1.0, 1.0, 0.5, ignore_index=ignore, class_weights=cw.tolist())
    s = 3.7
    s32 = float(torch.tensor(s, dtype=torch.float32))
    x = z.view(n, c, h, w).to(DEV).requires_grad_(True)
    out = crit(x, t.view(n, h, w).to(DEV))
    (s * out).backward()
    assert float(out) == float(loss[0])
    want = dl.double() * s32
    err = (x.grad.cpu().view(n, c, -1).double() - want).abs()
    assert bool((err <= 2.0 ** -24 * want.abs() + 2.0 ** -149).all()), float((err / want.abs().clamp_min(1e-300)).max())
    xb = z.view(n, c, h, w).to(DEV).bfloat16().requires_grad_(True)
    (s * crit(xb, t.view(n, h, w).to(DEV))).backward()
    assert xb.grad.dtype == torch.bfloat16 and torch.equal(xb.grad, x.grad.bfloat16())
