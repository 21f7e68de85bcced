"""Timing of the video frame kernels beside the uint8 RGB pair they stand next to: fdn_pre_yuv420 / fdn_post_yuv420 (yuv420p, nv12,
yuv420p10le) and fdn_pre_u8 / fdn_post_u8 on one batch of frames (default 8 x 720 x 1280 -> 736 x 1280) in one process.  HIP events
around windows of `--launches` back-to-back launches of one kernel, the kernels alternating round by round after a warm-up of every one
of them; reported per launch: the median and the least window, and the bytes the kernel has to move over the median.  Prints one JSON
line; --out writes it too.

    python tools/bench_yuv.py --out profiles/yuv_bench.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fdn-tip2025_amd")):
    sys.path.insert(0, p)
from fdn_hip import harness  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--launches", type=int, default=200, help="launches per timed window")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_yuv.py needs a ROCm GPU")
    dev = torch.device("cuda:0")
    h, w, B = a.height, a.width, a.batch
    H, W = harness.padded_size(h, w)
    g = torch.Generator().manual_seed(5)
    rgb = (torch.rand(B, h, w, 3, generator=g) * 255).to(torch.uint8).to(dev)
    res = (torch.rand(B, 3, H, W, generator=g) * 1.4 - 0.2).to(dev)
    fp32_in, fp32_out = B * 3 * H * W * 4, B * 3 * h * w * 4                  # pre writes the padded planes, post reads the crop
    jobs = {"fdn_pre_u8": (lambda: harness.preprocess(rgb, bgr=False), B * h * w * 3 + fp32_in),
            "fdn_post_u8": (lambda: harness.postprocess(res, h, w, bgr=False), fp32_out + B * h * w * 3)}
    for pix in ("yuv420p", "nv12", "yuv420p10le"):
        fmt = harness.VideoFormat(pix, "bt709", False, "left")
        n = fmt.frame_samples(h, w)
        frames = torch.randint(0, 2 ** fmt.bits, (B, n), generator=g).to(fmt.dtype).to(dev)
        jobs[f"fdn_pre_yuv420 {pix}"] = (lambda frames=frames, fmt=fmt: harness.preprocess_yuv420(frames, h, w, fmt), B * n * fmt.sample_bytes + fp32_in)
        jobs[f"fdn_post_yuv420 {pix}"] = (lambda fmt=fmt: harness.postprocess_yuv420(res, h, w, fmt), fp32_out + B * n * fmt.sample_bytes)
    for fn, _ in jobs.values():                                               # warm-up: code objects, the allocator's blocks
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    windows = {k: [] for k in jobs}
    for _ in range(a.rounds):
        for k, (fn, _) in jobs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            windows[k].append(e0.elapsed_time(e1) / a.launches)
    out = {"what": "per-launch time of the frame conversion kernels, HIP events around windows of back-to-back launches (allocation of the "
                   "output included)", "frames": [B, h, w], "padded": [H, W], "launches_per_window": a.launches, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "kernels": {}}
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
