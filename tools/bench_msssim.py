"""Multi-scale SSIM timing (fdn_hip.msssim, libfdn_msssim.so): one 720 x 1280 pair of 8-bit images in mode rgb and in mode gray, one 720p
luma pair at 8 and at 10 bit, and for scale the single-scale fdn_yuv420_ssim_y of the same 8-bit frame (--what).  After a warm-up,
`--reps` windows timed two ways: HIP events around `--inner` back-to-back enqueues of the launches alone (workspace and outputs allocated
once; the figure is the window over `--inner`), and wall clock around the call that returns Python numbers (with its allocations and the
copy back).  Prints one JSON line; --out merges it into that file under the key --what, so every case can run as a process of its own,
each under its own time limit:

    for w in rgb gray luma8 luma10 ssim_y; do timeout 300 python tools/bench_msssim.py --what $w --out profiles/msssim_bench.json || break; done
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fdn-tip2025_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_sharpness import events, frames  # noqa: E402
from fdn_hip import harness, msssim, ptr, stream, video_metrics  # noqa: E402

CASES = ("rgb", "gray", "luma8", "luma10", "ssim_y")


def luma_pair(B, h, w, bits, seed):
    """the Y planes of bench_sharpness.frames' green channels as 4:2:0 frames with grey chroma: [B][h*w*3/2] of the format's sample type"""
    gt, rs = frames(B, h, w, seed)
    out = []
    for t in (gt, rs):
        y = t[..., 1].reshape(B, h * w).to(torch.int16)
        if bits == 10:
            y = y * 4 + 1
        c = torch.full((B, h * w // 2), 1 << (bits - 1), dtype=torch.int16)
        f = torch.cat([y, c], dim=1)
        out.append(f.to(torch.uint8) if bits == 8 else f)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=CASES, required=True)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20, help="enqueues per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, h, w = a.batch, a.height, a.width
    l = msssim.lib()
    taps = ctypes.c_void_p(msssim._TAPS.ctypes.data)
    if a.what in ("rgb", "gray"):
        gt, rs = (t.to("cuda:0") for t in frames(B, h, w, 7))
        planes = 3 if a.what == "rgb" else 1
        ws = torch.empty(int(l.fdn_msssim_ws(B, planes, h, w)), dtype=torch.float64, device="cuda:0")
        out = torch.empty((B * planes, 5, 2), dtype=torch.float64, device="cuda:0")
        launch = lambda: l.fdn_msssim_u8(ptr(gt), ptr(rs), B, h, w, msssim.MODES[a.what], 0, taps, None, None, None, None, ptr(ws), ptr(out), stream())  # noqa: E731
        call = lambda: msssim.ms_ssim_u8(gt, rs, mode=a.what, bgr=False)      # noqa: E731
        first = lambda r: r[0]["ms_ssim"]      # noqa: E731
    else:
        bits = 10 if a.what == "luma10" else 8
        fmt = harness.VideoFormat("yuv420p10le" if bits == 10 else "yuv420p", "bt709", False, "left")
        fa, fb = (t.to("cuda:0") for t in luma_pair(B, h, w, bits, 7))
        if a.what == "ssim_y":
            from fdn_hip import lib
            ws = torch.empty(int(lib().fdn_yuv420_ssim_y_ws(B, h, w)), dtype=torch.float64, device="cuda:0")
            out = torch.empty(B, dtype=torch.float64, device="cuda:0")
            launch = lambda: lib().fdn_yuv420_ssim_y(ptr(fa), ptr(fb), ptr(out), ptr(ws), taps, B, h, w, bits, stream())      # noqa: E731
            call = lambda: video_metrics.ssim_y(fa, fb, h, w, fmt).cpu().tolist()      # noqa: E731
            first = lambda r: r[0]      # noqa: E731
        else:
            ws = torch.empty(int(l.fdn_msssim_ws(B, 1, h, w)), dtype=torch.float64, device="cuda:0")
            out = torch.empty((B, 5, 2), dtype=torch.float64, device="cuda:0")
            launch = lambda: l.fdn_msssim_luma(ptr(fa), ptr(fb), B, h, w, bits, h * w * 3 // 2, taps, None, None, None, None, ptr(ws), ptr(out), stream())  # noqa: E731
            call = lambda: msssim.ms_ssim_luma(fa, fb, h, w, fmt)      # noqa: E731
            first = lambda r: r[0]["ms_ssim"]      # noqa: E731
    for _ in range(a.warmup):
        res = call()
        assert launch() == 0
    torch.cuda.synchronize()
    wall = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
    gpu = events(launch, a.reps, a.inner)
    r = {"what": a.what, "batch": B, "height": h, "width": w, "reps": a.reps, "inner": a.inner,
         "gpu_ms_median": round(gpu[0], 4), "gpu_ms_min": round(gpu[1], 4), "gpu_ms_max": round(gpu[2], 4), "gpu_ms_per_pair": round(gpu[0] / B, 5),
         "wall_ms_median": round(1e3 * float(np.median(wall)), 3), "wall_ms_min": round(1e3 * min(wall), 3),
         "first": round(float(first(res)), 6), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(r))
    if a.out:
        have = {}
        if os.path.isfile(a.out):
            with open(a.out) as f:
                have = json.load(f)
        have[a.what] = r
        with open(a.out, "w") as f:
            f.write(json.dumps({k: have[k] for k in CASES if k in have}, indent=1) + "\n")


if __name__ == "__main__":
    main()
