"""Fourier evaluation timing: fourier_metrics on B pairs of 3 x 736 x 1280 planes (the 720p shape of the inference path).  After a warm-up,
`--reps` calls timed two ways: wall clock around a synchronised call (with the copy back and the host arithmetic), and HIP events around
the launches, whole (pair_bands: two rfft2 and the band sums) and in parts (one rfft2; the band sums on spectra already there).  Next to the
times, the bytes each part has to move at the least and the time that takes at --hbm-gbs.  Prints one JSON line; --out writes it too.

    python tools/bench_spectral.py --batch 8 --reps 20 --out profiles/spectral_bench.json
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
from fdn_hip import spectral  # noqa: E402


def frames(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    base = 0.4 + 0.2 * torch.sin(xx / 27.0) * torch.cos(yy / 33.0) + 0.1 * ((xx // 64 + yy // 48) % 2)
    x = torch.stack([base * 0.8 + 0.1, base, base * 0.9])[None] + 0.03 * torch.randn(B, 3, H, W, generator=g)
    return x.clamp(0, 1)


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
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=736)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--bands", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hbm-gbs", type=float, default=4000.0, help="the HBM rate the floors are stated against, GB/s")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, H, W = a.batch, a.height, a.width
    gt = frames(B, H, W, 7).to("cuda:0")
    rs = (0.85 * gt + 0.02 * torch.randn(gt.shape, generator=torch.Generator().manual_seed(8)).to("cuda:0")).clamp(0, 1)
    for _ in range(a.warmup):
        m = spectral.fourier_metrics(rs, gt, a.bands)
    torch.cuda.synchronize()
    wall = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        m = spectral.fourier_metrics(rs, gt, a.bands)
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
    za, zb = spectral.rfft2(rs), spectral.rfft2(gt)
    whole = events(lambda: spectral.pair_bands(rs, gt, a.bands), a.reps)
    fft = events(lambda: spectral.rfft2(rs), a.reps)
    sums = events(lambda: spectral.spectrum_pair_bands(za, zb, H, W, a.bands), a.reps)
    planes, Wf = B * 3, W // 2 + 1
    real, spec = planes * H * W * 4, planes * H * Wf * 8
    # one rfft2: rows read the image and write the spectrum, columns read and write it; the sums read both spectra once
    bytes_fft, bytes_sums = real + 3 * spec, 2 * spec
    floor = lambda n: round(n / (a.hbm_gbs * 1e9) * 1e3, 4)
    r = {"what": "fourier_metrics", "batch": B, "height": H, "width": W, "bands": a.bands, "reps": a.reps,
         "wall_ms_median": round(1e3 * float(np.median(wall)), 3), "wall_ms_min": round(1e3 * min(wall), 3),
         "gpu_ms_median": round(whole[0], 3), "gpu_ms_min": round(whole[1], 3), "gpu_ms_per_pair": round(whole[0] / B, 4),
         "rfft2_ms_median": round(fft[0], 3), "band_sums_ms_median": round(sums[0], 3),
         "bytes_rfft2": bytes_fft, "bytes_band_sums": bytes_sums, "bytes_whole": 2 * bytes_fft + bytes_sums,
         "hbm_gbs": a.hbm_gbs, "floor_ms_rfft2": floor(bytes_fft), "floor_ms_band_sums": floor(bytes_sums),
         "floor_ms_whole": floor(2 * bytes_fft + bytes_sums),
         "times_floor_whole": round(whole[0] / (floor(2 * bytes_fft + bytes_sums) or 1), 1),
         "times_floor_band_sums": round(sums[0] / (floor(bytes_sums) or 1), 1),
         "pairs_per_s": round(B / float(np.median(wall)), 1),
         "first": {k: (round(v, 6) if isinstance(v, float) else v) for k, v in m[0].items() if k != "bands"},
         "device": torch.cuda.get_device_name(0)}
    print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(r, indent=1) + "\n")


if __name__ == "__main__":
    main()
