"""Low-light evaluation timing: one of LOE on the size-50 grid, LOE at full resolution, dE00, dE00 with its map (--what), on B pairs of
h x w 8-bit images.  After a warm-up, `--reps` calls timed two ways: HIP events around the launches, and wall clock around the call that
returns Python numbers (with the copy back).  Next to the times, the bytes the two images hold and the time reading them from HBM would
take at --hbm-gbs (every repetition reads the same buffers, which at the default size fit the Infinity Cache: the inputs are warm).
Prints one JSON line; --out merges it into that file under the key --what, so every case can run as a process of its own, each under
its own time limit:

    for w in loe50 loe0 deltae deltae_map; do timeout 300 python tools/bench_lowlight.py --what $w --out profiles/lowlight_bench.json || break; done
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
from fdn_hip import lowlight  # noqa: E402

CASES = ("loe50", "loe0", "deltae", "deltae_map")


def frames(B, h, w, seed):
    """a dark, textured batch and a brightened noisy version of it, uint8 [B][h][w][3]"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    base = 0.08 + 0.05 * torch.sin(xx / 27.0) * torch.cos(yy / 33.0) + 0.03 * ((xx // 64 + yy // 48) % 2)
    dark = (torch.stack([base * 0.8, base, base * 0.9], -1)[None] + 0.01 * torch.randn(B, h, w, 3, generator=g)).clamp(0, 1)
    lit = (dark * 5.0 + 0.03 * torch.randn(B, h, w, 3, generator=g)).clamp(0, 1)
    return (dark * 255).round().to(torch.uint8), (lit * 255).round().to(torch.uint8)


def events(f, reps):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out)), min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=CASES, required=True)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hbm-gbs", type=float, default=4000.0, help="the HBM rate the floor is stated against, GB/s")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, h, w = a.batch, a.height, a.width
    dark, lit = (t.to("cuda:0") for t in frames(B, h, w, 7))
    if a.what.startswith("loe"):
        size = 50 if a.what == "loe50" else 0
        out = torch.empty((B, 2), dtype=torch.int64, device="cuda:0")
        launch = lambda: lowlight._loe_launch(dark, lit, size, out)
        call = lambda: lowlight.loe_u8(dark, lit, size)
    else:
        want_map = a.what == "deltae_map"
        out = torch.empty((B, 2), dtype=torch.float64, device="cuda:0")
        launch = lambda: lowlight._deltae_launch(lit, dark, False, out, want_map)
        call = lambda: lowlight.deltae00_u8(lit, dark, bgr=False, want_map=want_map)
    for _ in range(a.warmup):
        first = call()
    torch.cuda.synchronize()
    wall = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
    gpu = events(launch, a.reps)
    nbytes = 2 * B * h * w * 3                                        # both images read once (a sampled LOE touches less of them)
    floor = nbytes / (a.hbm_gbs * 1e9) * 1e3
    r = {"what": a.what, "batch": B, "height": h, "width": w, "reps": a.reps,
         "gpu_ms_median": round(gpu[0], 4), "gpu_ms_min": round(gpu[1], 4), "gpu_ms_per_pair": round(gpu[0] / B, 5),
         "wall_ms_median": round(1e3 * float(np.median(wall)), 3), "wall_ms_min": round(1e3 * min(wall), 3),
         "bytes_images": nbytes, "hbm_gbs": a.hbm_gbs, "floor_ms_images": round(floor, 4), "times_floor": round(gpu[0] / floor, 1),
         "first": [round(float(v), 6) for v in (first if a.what.startswith("loe") else first[0])][:2],
         "device": torch.cuda.get_device_name(0)}
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
