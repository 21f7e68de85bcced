"""PIQE timing (fdn_hip.piqe, libfdn_piqe.so): one 720 x 1280 8-bit image, a batch of eight, one 720p luma plane at 8 and at 10 bit, and
for scale, from the same run, the single-scale fdn_yuv420_ssim_y of the same 8-bit frame against itself and the launches of NIQE
(metrics.niqe_features) on the same frame.  After a warm-up, `--reps` windows timed two ways: HIP events around `--inner` back-to-back
enqueues of the launches alone (workspace and outputs allocated once; the figure is the window over `--inner`), and wall clock around the
call that returns Python numbers (with its allocations and the copy back).  `read_us` is the time one read of the input would take at
--hbm-gbs: the bytes PIQE must move.  One process runs every case and writes them together:

    timeout 300 python tools/bench_piqe.py --out profiles/piqe_bench.json
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
from fdn_hip import harness, metrics, piqe, ptr, stream, video_metrics  # noqa: E402

CASES = ("u8", "u8_batch8", "luma8", "luma10", "ssim_y", "niqe")


def luma_frames(B, h, w, bits, seed):
    """the Y planes of bench_sharpness.frames' restored green channels as 4:2:0 frames with grey chroma: [B][h*w*3/2]"""
    y = frames(B, h, w, seed)[1][..., 1].reshape(B, h * w).to(torch.int16)
    if bits == 10:
        y = y * 4 + 1
    f = torch.cat([y, torch.full((B, h * w // 2), 1 << (bits - 1), dtype=torch.int16)], dim=1)
    return f.to(torch.uint8) if bits == 8 else f


def case(what, h, w):
    """-> (launch, call, first, batch, input bytes)"""
    l = piqe.lib()
    taps = ctypes.c_void_p(piqe._TAPS.ctypes.data)
    if what in ("u8", "u8_batch8"):
        B = 8 if what == "u8_batch8" else 1
        x = frames(B, h, w, 7)[1].to("cuda:0")
        ws = torch.empty(int(l.fdn_piqe_ws(B, h, w)), dtype=torch.float64, device="cuda:0")
        out = torch.empty((B, 2), dtype=torch.float64, device="cuda:0")
        return (lambda: l.fdn_piqe_u8(ptr(x), B, h, w, 0, taps, None, None, None, ptr(ws), ptr(out), stream()),
                lambda: piqe.piqe_u8(x), lambda r: r[0]["piqe"], B, B * h * w * 3)
    if what == "niqe":
        x = frames(1, h, w, 7)[1].to("cuda:0").permute(0, 3, 1, 2).flip(1).float().contiguous()       # B, G, R planes in [0, 255]
        window = metrics.niqe_params(os.path.join(ROOT, "tests", "golden", "niqe_pris_params.npz"))[2]
        f = lambda: metrics.niqe_features(x, window=window)      # noqa: E731
        return (lambda: (f(), 0)[1]), f, lambda r: float(r["feats"].flatten()[0]), 1, h * w * 3 * 4      # five launches, outputs allocated per call
    bits = 10 if what == "luma10" else 8
    fmt = harness.VideoFormat("yuv420p10le" if bits == 10 else "yuv420p", "bt709", False, "left")
    f = luma_frames(1, h, w, bits, 7).to("cuda:0")
    if what == "ssim_y":
        from fdn_hip import lib
        from fdn_hip.metrics import ssim3d_taps
        t11 = np.ascontiguousarray(ssim3d_taps(), dtype=np.float64)
        ws = torch.empty(int(lib().fdn_yuv420_ssim_y_ws(1, h, w)), dtype=torch.float64, device="cuda:0")
        out = torch.empty(1, dtype=torch.float64, device="cuda:0")
        return (lambda: lib().fdn_yuv420_ssim_y(ptr(f), ptr(f), ptr(out), ptr(ws), ctypes.c_void_p(t11.ctypes.data), 1, h, w, bits, stream()),
                lambda: video_metrics.ssim_y(f, f, h, w, fmt).cpu().tolist(), lambda r: r[0], 1, 2 * h * w)
    ws = torch.empty(int(l.fdn_piqe_ws(1, h, w)), dtype=torch.float64, device="cuda:0")
    out = torch.empty((1, 2), dtype=torch.float64, device="cuda:0")
    return (lambda: l.fdn_piqe_luma(ptr(f), 1, h, w, bits, h * w * 3 // 2, taps, None, None, None, ptr(ws), ptr(out), stream()),
            lambda: piqe.piqe_luma(f, h, w, fmt), lambda r: r[0]["piqe"], 1, h * w * (2 if bits == 10 else 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=CASES, nargs="*", default=list(CASES))
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20, help="enqueues per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hbm-gbs", type=float, default=4000.0, help="the HBM rate the one-read time is stated against, GB/s")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    h, w = a.height, a.width
    res = {}
    for what in a.what:
        launch, call, first, B, nbytes = case(what, h, w)
        for _ in range(a.warmup):
            r = call()
            assert launch() == 0
        torch.cuda.synchronize()
        wall = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
        gpu = events(launch, a.reps, a.inner)
        res[what] = {"what": what, "batch": B, "height": h, "width": w, "reps": a.reps, "inner": a.inner,
                     "gpu_ms_median": round(gpu[0], 4), "gpu_ms_min": round(gpu[1], 4), "gpu_ms_max": round(gpu[2], 4),
                     "gpu_ms_per_image": round(gpu[0] / B, 5), "wall_ms_median": round(1e3 * float(np.median(wall)), 3),
                     "wall_ms_min": round(1e3 * min(wall), 3), "input_bytes": nbytes, "read_us": round(nbytes / (a.hbm_gbs * 1e3), 3),
                     "first": round(float(first(r)), 6), "device": torch.cuda.get_device_name(0)}
        print(json.dumps(res[what]), flush=True)
    if a.out:
        have = {}
        if os.path.isfile(a.out):
            with open(a.out) as f:
                have = json.load(f)
        have.update(res)
        with open(a.out, "w") as f:
            f.write(json.dumps({k: have[k] for k in CASES if k in have}, indent=1) + "\n")


if __name__ == "__main__":
    main()
