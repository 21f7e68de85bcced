"""Deblurring evaluation timing: one of the plain paired scores (fdn_hip.metrics.calculate_psnr_ssim_u8), the edge error, GMSD with the
mean gradients, and the three figures together (--what), on B pairs of h x w 8-bit images.  After a warm-up, `--reps` windows timed two
ways: HIP events around `--inner` back-to-back enqueues of the launches alone (workspace and outputs allocated once; the figure is the
window over `--inner`), and wall clock around the call that returns Python numbers (with its allocations and the copy back).  Next to the
times, the bytes the two images hold and the time reading them from HBM would take at --hbm-gbs (every repetition reads the same
buffers, which at the default size fit the Infinity Cache: the inputs are warm).  Prints one JSON line; --out merges it into that file
under the key --what, so every case can run as a process of its own, each under its own time limit:

    for w in plain edge gmsd all; do timeout 300 python tools/bench_sharpness.py --what $w --out profiles/sharpness_bench.json || break; done
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fdn-tip2025_amd"))
from fdn_hip import metrics, sharpness  # noqa: E402

CASES = ("plain", "edge", "gmsd", "all")


def frames(B, h, w, seed):
    """a textured ground truth and a softer, darker, noisy restored version of it, uint8 [B][h][w][3]"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    base = 0.45 + 0.2 * torch.sin(xx / 7.0) * torch.cos(yy / 9.0) + 0.1 * ((xx // 16 + yy // 12) % 2)
    gt = (torch.stack([base * 0.9, base, base * 1.1], -1)[None] + 0.05 * torch.randn(B, h, w, 3, generator=g)).clamp(0, 1)
    soft = torch.nn.functional.avg_pool2d(gt.permute(0, 3, 1, 2), 3, stride=1, padding=1, count_include_pad=False).permute(0, 2, 3, 1)
    rs = (soft * 0.8 + 0.03 + 0.01 * torch.randn(B, h, w, 3, generator=g)).clamp(0, 1)
    return (gt * 255).round().to(torch.uint8), (rs * 255).round().to(torch.uint8)


def events(f, reps, inner):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            f()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / inner)
    return float(np.median(out)), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=CASES, required=True)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20, help="enqueues per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hbm-gbs", type=float, default=4000.0, help="the HBM rate the floor is stated against, GB/s")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, h, w = a.batch, a.height, a.width
    gt, rs = (t.to("cuda:0") for t in frames(B, h, w, 7))
    from fdn_hip import lib, ptr, stream
    if a.what == "plain":
        nws = int(lib().fdn_pair_ssim3d_ws(B, h, w, 0))
        stats = torch.empty((B, metrics.PAIR_PARTS, 2), dtype=torch.int64, device="cuda:0")
        ws = torch.empty(nws, dtype=torch.float64, device="cuda:0")
        out = torch.empty((B, 3), dtype=torch.float64, device="cuda:0")
        taps, mix = metrics.ssim3d_taps(), np.ascontiguousarray(metrics.ssim3d_channel_matrix())
        tp, mp = taps.ctypes.data, mix.ctypes.data

        def launch():
            lib().fdn_pair_sse_u8(ptr(gt), ptr(rs), B, h, w, 0, ptr(stats), stream())
            lib().fdn_pair_ssim3d_u8(ptr(gt), ptr(rs), B, h, w, 0, ptr(stats), tp, mp, ptr(ws), ptr(out), stream())
        call = lambda: metrics.calculate_psnr_ssim_u8(gt, rs, bgr=False)
        passes = 2                                                    # the squared differences, then the tiles
        first = lambda r: [float(r[0][0]), float(r[1][0])]
    else:
        l = sharpness.lib()
        ews = torch.empty(int(l.fdn_edge_ws(B, h, w)), dtype=torch.float64, device="cuda:0")
        gws = torch.empty(int(l.fdn_gmsd_ws(B, h, w)), dtype=torch.float64, device="cuda:0")
        out = torch.empty(5 * B, dtype=torch.float64, device="cuda:0")

        def edge():
            l.fdn_edge_u8(ptr(gt), ptr(rs), B, h, w, None, ptr(ews), ptr(out), stream())

        def gmsd():
            l.fdn_gmsd_u8(ptr(gt), ptr(rs), B, h, w, 0, None, None, ptr(gws), ptr(out[B:]), stream())
        if a.what == "edge":
            launch, call, passes = edge, lambda: sharpness.edge_error_u8(gt, rs), 1
            first = lambda r: [float(r[0])]
        elif a.what == "gmsd":
            launch, call, passes = gmsd, lambda: sharpness.gmsd_u8(gt, rs, bgr=False), 1
            first = lambda r: [float(r[0])]
        else:
            launch, call, passes = lambda: (edge(), gmsd()), lambda: sharpness.sharpness_metrics(gt, rs, bgr=False), 2
            first = lambda r: [r[0][k] for k in ("edge", "gmsd", "grad_ratio")]
    for _ in range(a.warmup):
        res = call()
        launch()
    torch.cuda.synchronize()
    wall = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
    gpu = events(launch, a.reps, a.inner)
    nbytes = 2 * B * h * w * 3                                        # both images, read once per pass (the tiles read their aprons besides)
    floor = passes * nbytes / (a.hbm_gbs * 1e9) * 1e3
    r = {"what": a.what, "batch": B, "height": h, "width": w, "reps": a.reps, "inner": a.inner,
         "gpu_ms_median": round(gpu[0], 4), "gpu_ms_min": round(gpu[1], 4), "gpu_ms_max": round(gpu[2], 4), "gpu_ms_per_pair": round(gpu[0] / B, 5),
         "wall_ms_median": round(1e3 * float(np.median(wall)), 3), "wall_ms_min": round(1e3 * min(wall), 3),
         "wall_ms_per_pair": round(1e3 * float(np.median(wall)) / B, 4),
         "bytes_images": nbytes, "passes": passes, "hbm_gbs": a.hbm_gbs, "floor_ms_images": round(floor, 4), "times_floor": round(gpu[0] / floor, 1),
         "first": [round(v, 6) for v in first(res)],
         "device": torch.cuda.get_device_name(0)}
    print(json.dumps(r))
    if a.out:
        have = {}
        if os.path.isfile(a.out):
            with open(a.out) as f:
                have = json.load(f)
        have[a.what] = r
        if "plain" in have:
            for k in CASES[1:]:
                if k in have:
                    have[k]["gpu_ratio_to_plain"] = round(have[k]["gpu_ms_median"] / have["plain"]["gpu_ms_median"], 3)
                    have[k]["wall_ratio_to_plain"] = round(have[k]["wall_ms_median"] / have["plain"]["wall_ms_median"], 3)
        with open(a.out, "w") as f:
            f.write(json.dumps({k: have[k] for k in CASES if k in have}, indent=1) + "\n")


if __name__ == "__main__":
    main()
