#!/usr/bin/env python3
"""Micro-benchmark of the map-smoothing kernel (csrc/smooth.hip) at sigma 4 (radius 16), timed with events in one
process next to a torch copy of the same byte count and next to the torch composition it replaces (reflect pad, two
F.conv2d, amax): microseconds, achieved GB/s on the algorithmic bytes, and the two ratios.

    python tools/bench_smooth.py [--iters 50] [--sigma 4] [--out profiles/smooth_bench.txt]

Bytes of the kernel = one plane read + one plane written per image (+ 4 per image for the maximum); the copy moves the
same number (half read, half written).  The kernel time is the C-ABI call alone (image_max fill + kernel); the whole
call adds GaussianSmoother's allocations.  The torch composition pads by the radius with mode="reflect" where the sides
allow (torch's reflect differs from scipy's at the border, which does not change its cost) in one F.pad, then runs a
1 x K and a K x 1 convolution and amax.
"""
import argparse
import ctypes as C
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tiaozhanbei_unet_amd import _lib as L  # noqa: E402
from tiaozhanbei_unet_amd.evaluation import GaussianSmoother  # noqa: E402
from tools.bench_stream import timeit  # noqa: E402

SHAPES = [(32, 256, 256), (8, 1408, 512)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--sigma", type=float, default=4.0)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "smooth_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lib = L.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    sm = GaussianSmoother(a.sigma)
    r = sm.radius
    lines = [f"# tools/bench_smooth.py --iters {a.iters} --sigma {a.sigma} (radius {r}) on {torch.cuda.get_device_name(0)}: "
             "event times, mean per launch"]
    full = torch.from_numpy(sm.taps).to(dev)
    full = torch.cat([full.flip(0)[:-1], full])
    kw, kh = full.reshape(1, 1, 1, -1), full.reshape(1, 1, -1, 1)
    for n, h, w in SHAPES:
        maps = torch.rand((n, 1, h, w), device=dev)
        out = torch.empty_like(maps)
        peak = torch.empty(n, device=dev)

        def kernel():
            L.check(lib.unet_smooth_maps(p(maps), p(out), n, h, w, sm._host, r, p(peak), st), "smooth")

        def composition():
            x = F.pad(maps, (r, r, r, r), mode="reflect")
            y = F.conv2d(F.conv2d(x, kw), kh)
            return y, y.amax((1, 2, 3))

        nbytes = n * h * w * 8 + n * 4
        src = torch.empty(nbytes // 8, dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        t_copy = timeit(lambda: dst.copy_(src), a.iters)
        t_kern = timeit(kernel, a.iters)
        t_call = timeit(lambda: sm(maps), a.iters)
        t_torch = timeit(composition, a.iters)
        y, m = composition()
        sm_out, sm_peak = sm(maps)
        inner = (slice(None), slice(None), slice(r, h - r), slice(r, w - r))       # (the borders differ by definition)
        diff = float((y[inner] - sm_out[inner]).abs().max())
        lines.append(f"{n}x{h}x{w}: {nbytes / 1e6:.1f} MB | smooth kernel {t_kern * 1e3:.1f} us {nbytes / t_kern / 1e6:.0f} GB/s | "
                     f"torch copy of the same bytes {t_copy * 1e3:.1f} us {nbytes / t_copy / 1e6:.0f} GB/s | kernel / copy "
                     f"{t_kern / t_copy:.2f} | torch composition (pad, 2 conv2d, amax) {t_torch * 1e3:.1f} us | composition / "
                     f"kernel {t_torch / t_kern:.2f} | whole GaussianSmoother call {t_call * 1e3:.1f} us | max interior "
                     f"difference to the composition {diff:.2e}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
