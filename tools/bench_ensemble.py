"""Timing of the self-ensemble kernels (include/fdn_ensemble.h): for each entry point the four codes that transpose (mask 0xF0, through the
LDS tile) beside the four that do not (mask 0x0F, along rows) - the same bytes moved, so the untransposed call is the baseline - and
fdn_pre_u8 / fdn_post_u8 beside them, on one batch of frames (default 720 x 1280, run it with --batch 1 and --batch 8) in one process.
HIP events around windows of `--launches` back-to-back launches of one kernel into buffers allocated once, the kernels alternating round
by round after a warm-up of every one of them; reported per launch: the median, the least and the largest window, and the bytes the
kernel has to move over the median.  Prints one JSON line; --out writes it too.

    python tools/bench_ensemble.py --batch 8 --out profiles/ensemble_bench.json
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fdn-tip2025_amd")):
    sys.path.insert(0, p)
import fdn_hip  # noqa: E402
from fdn_hip import harness  # noqa: E402


def make_jobs(B, h, w):
    """{name: (launch, bytes the kernel has to move)} and the two padded sizes"""
    dev = torch.device("cuda:0")
    lib, st = fdn_hip.lib(), fdn_hip.stream
    size = {0x0F: harness.padded_size(h, w), 0xF0: harness.padded_size(w, h)}
    g = torch.Generator().manual_seed(5)
    rgb = (torch.rand(B, h, w, 3, generator=g) * 255).to(torch.uint8).to(dev)
    x = torch.rand(B, 3, h, w, generator=g).to(dev)
    res = {m: (torch.rand(4, B, 3, *size[m], generator=g) * 1.4 - 0.2).to(dev) for m in size}
    copies = {m: torch.empty(4, B, 3, *size[m], device=dev) for m in size}
    mean = torch.empty(B, 3, h, w, device=dev)
    u8 = torch.empty(B, h, w, 3, device=dev, dtype=torch.uint8)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    n_u8, n_f32 = B * h * w * 3, B * 3 * h * w * 4
    jobs = {}
    for m, name in ((0x0F, "rows"), (0xF0, "transposed")):
        H, W = size[m]
        n_copies, n_crop = 4 * B * 3 * H * W * 4, 4 * n_f32               # the copies are written padded; the mean reads the crop
        ra, rb, dims = (p(res[m]), None, (H, W, 0, 0)) if m == 0x0F else (None, p(res[m]), (0, 0, H, W))
        jobs[f"fdn_d4_pre_u8 {name}"] = (lambda m=m, H=H, W=W: lib.fdn_d4_pre_u8(p(rgb), p(copies[m]), B, h, w, H, W, m, 0, st()),
                                         4 * n_u8 + n_copies)
        jobs[f"fdn_d4_apply {name}"] = (lambda m=m, H=H, W=W: lib.fdn_d4_apply(p(x), p(copies[m]), B, h, w, H, W, m, st()),
                                        4 * n_f32 + n_copies)
        jobs[f"fdn_d4_mean {name}"] = (lambda m=m, ra=ra, rb=rb, dims=dims: lib.fdn_d4_mean(ra, rb, p(mean), B, h, w, *dims, m, st()),
                                       n_crop + n_f32)
        jobs[f"fdn_d4_post_u8 {name}"] = (lambda m=m, ra=ra, rb=rb, dims=dims: lib.fdn_d4_post_u8(ra, rb, p(u8), B, h, w, *dims, m, 0, st()),
                                          n_crop + n_u8)
    H, W = size[0x0F]
    one = copies[0x0F][0]
    jobs["fdn_pre_u8"] = (lambda: lib.fdn_pre_u8(p(rgb), p(one), B, h, w, H, W, 0, st()), n_u8 + B * 3 * H * W * 4)
    jobs["fdn_post_u8"] = (lambda: lib.fdn_post_u8(p(res[0x0F]), p(u8), B, h, w, H, W, 0, st()), n_f32 + n_u8)
    return jobs, size


def time_jobs(jobs, launches, rounds):
    """{name: [ms per launch of each window]}"""
    for k, (fn, _) in jobs.items():                                           # warm-up: code objects; every call must be accepted
        for _ in range(10):
            fdn_hip.check(fn(), k)
    torch.cuda.synchronize()
    windows = {k: [] for k in jobs}
    for _ in range(rounds):
        for k, (fn, _) in jobs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            windows[k].append(e0.elapsed_time(e1) / launches)
    return windows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--launches", type=int, default=100, help="launches per timed window")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ensemble.py needs a ROCm GPU")
    h, w, B = a.height, a.width, a.batch
    jobs, size = make_jobs(B, h, w)
    windows = time_jobs(jobs, a.launches, a.rounds)
    out = {"what": "per-launch time of the self-ensemble kernels, HIP events around windows of back-to-back launches into buffers "
                   "allocated once; 'rows' = mask 0x0F, 'transposed' = mask 0xF0, four copies each",
           "frames": [B, h, w], "padded": {"rows": list(size[0x0F]), "transposed": list(size[0xF0])},
           "launches_per_window": a.launches, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "kernels": {}}
    for k, (_, nbytes) in jobs.items():
        med = float(np.median(windows[k]))
        out["kernels"][k] = {"ms_median": round(med, 4), "ms_min": round(min(windows[k]), 4), "ms_max": round(max(windows[k]), 4),
                             "bytes": nbytes, "GB_per_s_at_median": round(nbytes / med / 1e6, 1)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
