"""Paired-metrics timing: PSNR and 3-D SSIM of B uint8 pairs of 720 x 1280 resident on the device, two ways, alternating:
  batched : metrics.calculate_psnr_ssim_u8 on the uint8 batch (two launches and a finish, one device-to-host copy);
  route   : what there was before it - the bytes to float32 planes, then calculate_psnr and calculate_ssim image by image (three host
            synchronisations per image, the 3-D SSIM as three launches through a 10 x numel float32 work space).
After a warm-up of both, `--reps` repetitions of each, wall clock around a call that ends in a device synchronise.  Prints both series
and the largest difference between the two ways' scores; --out writes the same text.

    python tools/bench_paired_metrics.py --batch 8 --reps 5 --out profiles/r11_paired_metrics.txt
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fdn-tip2025_amd"))
from fdn_hip import metrics  # noqa: E402


def frames(B, H, W):
    g = torch.Generator().manual_seed(7)
    a = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.int32)
    b = (a + torch.randint(-20, 21, a.shape, generator=g, dtype=torch.int32)).clamp(0, 255)
    return a.to(torch.uint8), b.to(torch.uint8)


def route(a, b):
    psnr, ssim = [], []
    for i in range(a.shape[0]):
        x, y = a[i].permute(2, 0, 1).to(torch.float32).contiguous(), b[i].permute(2, 0, 1).to(torch.float32).contiguous()
        psnr.append(metrics.calculate_psnr(x, y))
        ssim.append(metrics.calculate_ssim(x, y))
    return psnr, ssim


def timed(fn, a, b):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn(a, b)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    a, b = (t.to("cuda:0") for t in frames(args.batch, args.height, args.width))
    for _ in range(args.warmup):
        route(a, b)
        metrics.calculate_psnr_ssim_u8(a, b)
    t_new, t_old = [], []
    for _ in range(args.reps):
        t, old = timed(route, a, b)
        t_old.append(t)
        t, new = timed(metrics.calculate_psnr_ssim_u8, a, b)
        t_new.append(t)
    lines = [f"paired metrics, {args.batch} pairs of {args.height} x {args.width} uint8 on {torch.cuda.get_device_name(0)}; wall ms per call, device synchronised",
             "route (float planes, calculate_psnr + calculate_ssim per image): " + " ".join(f"{t:.3f}" for t in t_old),
             "batched (calculate_psnr_ssim_u8):                                 " + " ".join(f"{t:.3f}" for t in t_new),
             f"slowest batched {max(t_new):.3f} ms, fastest route {min(t_old):.3f} ms: {min(t_old) / max(t_new):.1f}x",
             f"largest difference of the scores: PSNR {max(abs(p - q) for p, q in zip(old[0], new[0])):.2e} dB, "
             f"SSIM {max(abs(p - q) for p, q in zip(old[1], new[1])):.2e}"]
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
