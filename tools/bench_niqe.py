"""NIQE timing: calculate_niqe on B frames of 736 x 1280 (the 720p shape of the inference path) - the five launches, the copy back of the
features and the host MVG fit (nanmean, cov, pinv) per frame.  After a warm-up, `--reps` calls timed two ways: wall clock around a
synchronised call, and HIP events around the launches alone (niqe_features).  Prints one JSON line; --out writes it too.

    python tools/bench_niqe.py --batch 8 --reps 20 --out profiles/niqe_bench.json
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
from fdn_hip import metrics  # noqa: E402


def frames(B, H, W):
    g = torch.Generator().manual_seed(7)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    base = 100 + 50 * torch.sin(xx / 27.0) * torch.cos(yy / 33.0) + 30 * ((xx // 64 + yy // 48) % 2)
    x = torch.stack([base * 0.8 + 20, base, base * 0.9])[None] + 6 * torch.randn(B, 3, H, W, generator=g)
    return x.clamp(0, 255).round()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=736)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--params", default=os.path.join(ROOT, "tests", "golden", "niqe_pris_params.npz"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    params = metrics.niqe_params(a.params)
    p = {"mu_pris_param": params[0], "cov_pris_param": params[1], "gaussian_window": params[2]}
    x = frames(a.batch, a.height, a.width).to("cuda:0")
    for _ in range(a.warmup):
        metrics.calculate_niqe(x, params=p)
    torch.cuda.synchronize()
    wall = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        q = metrics.calculate_niqe(x, params=p)
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
    ev = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        metrics.niqe_features(x, window=params[2])
        e1.record()
        torch.cuda.synchronize()
        ev.append(e0.elapsed_time(e1))
    r = {"what": "calculate_niqe", "batch": a.batch, "height": a.height, "width": a.width, "reps": a.reps,
         "wall_ms_median": round(1e3 * float(np.median(wall)), 3), "wall_ms_min": round(1e3 * min(wall), 3),
         "gpu_ms_median": round(float(np.median(ev)), 3), "gpu_ms_min": round(min(ev), 3),
         "frames_per_s": round(a.batch / float(np.median(wall)), 1), "scores": [round(s, 6) for s in (q if isinstance(q, list) else [q])],
         "device": torch.cuda.get_device_name(0)}
    print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(r, indent=1) + "\n")


if __name__ == "__main__":
    main()
