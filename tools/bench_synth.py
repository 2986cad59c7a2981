#!/usr/bin/env python3
"""Micro-benchmark of the synthetic-anomaly kernel (csrc/synth.hip) next to a torch copy of the same byte count, timed
with events in the same process: microseconds, achieved TB/s and the ratio of the two times.

    python tools/bench_synth.py [--iters 50] [--out profiles/synth_bench.txt]

Bytes of the kernel = 3 planes read + 3 planes and 1 mask written + 3 donor reads per masked pixel (the measured mask
coverage); the copy moves the same number (half read, half written).  Every image is corrupted (p = 1), the parameters
are AnomalySynthesizer's own draws at threshold 0.5.
"""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tiaozhanbei_unet_amd import _lib as L, augment as A  # noqa: E402
from tools.bench_stream import timeit  # noqa: E402

SHAPES = [(32, 256, 256), (8, 512, 512)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "synth_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lib = L.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    lines = [f"# tools/bench_synth.py --iters {a.iters} on {torch.cuda.get_device_name(0)}: event times, p = 1, threshold 0.5"]
    for n, h, w in SHAPES:
        images = torch.randn((n, 3, h, w), device=dev)
        synth = A.AnomalySynthesizer(p=1.0, threshold=0.5, seed=1)
        params = synth.draw(n, (h, w))
        desc = synth.table(params)
        corrupted, masks = synth(images, params=params)
        cover = float(masks.mean())
        desc_dev = torch.from_numpy(desc.view("u1").reshape(n, -1)).to(dev)
        (ycell, ytf), (xcell, xtf) = A._synth_axis_tables(h, dev), A._synth_axis_tables(w, dev)
        grad = A._synth_gradients(dev)

        def kernel():
            L.check(lib.unet_synth_anomalies(p(images), None, n, 3, h, w, p(desc_dev), desc.ctypes.data_as(C.c_void_p),
                                             p(ycell), p(ytf), p(xcell), p(xtf), p(grad), p(corrupted), p(masks), st), "synth")

        nbytes = int(n * h * w * 4 * (7 + 3 * cover))
        src = torch.empty(nbytes // 8, dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        t_copy = timeit(lambda: dst.copy_(src), a.iters)
        t_kern = timeit(kernel, a.iters)
        t_call = timeit(lambda: synth(images, params=params), a.iters)
        lines.append(f"{n}x3x{h}x{w}: mask covers {100 * cover:.1f} %, {nbytes / 1e6:.1f} MB | synth kernel {t_kern * 1e3:.1f} us "
                     f"{nbytes / t_kern / 1e9:.2f} TB/s | torch copy of the same bytes {t_copy * 1e3:.1f} us "
                     f"{nbytes / t_copy / 1e9:.2f} TB/s | ratio {t_kern / t_copy:.2f} | whole call with host set-up "
                     f"{t_call * 1e3:.1f} us")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
