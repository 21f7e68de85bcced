"""LPIPS timing: fdn_hip.lpips.LPIPS on B pairs of 736 x 1280 (the 720p shape of the inference path) for both backbones, with seeded
random weights (tests/lpips_ref.py; the time does not depend on the values).  After a warm-up, `--reps` calls timed two ways: wall clock
around a synchronised call (scaling layer, backbone over the 2B images, five heads, the copy of the [B] scores back), and HIP events
around the launches alone.  The backbone's conv FLOP are counted from the shapes.  Prints one JSON line; --out writes it too.

    python tools/bench_lpips.py --batch 4 --reps 10 --out profiles/lpips_bench.json
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lpips_ref as R  # noqa: E402
from fdn_hip import lpips  # noqa: E402


def conv_gflop(net, H, W):
    """multiply-adds x 2 of the backbone's convs for one H x W image"""
    h, w, fl = H, W, 0
    for op in lpips.ARCH[net]:
        if op[0] == "conv":
            _, _, cin, cout, k, s, p = op
            h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
            fl += 2 * cout * cin * k * k * h * w
        elif op[0] == "pool":
            h, w = (h - op[1]) // op[2] + 1, (w - op[1]) // op[2] + 1
    return fl / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4, help="pairs per call (the backbone runs on 2 x batch images)")
    ap.add_argument("--height", type=int, default=736)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nets", default="vgg,alex")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    x = R.images(a.batch, a.height, a.width, seed=7)
    y = R.distorted(x, "distinct", seed=8)
    x, y = x.to("cuda:0"), y.to("cuda:0")
    res = {"what": "fdn_hip.lpips.LPIPS", "batch_pairs": a.batch, "height": a.height, "width": a.width, "reps": a.reps}
    for net in a.nets.split(","):
        p = R.make_params(net, 0)
        m = lpips.LPIPS(net, weights=R.lpips_state_dict(net, p), device="cuda:0")
        for _ in range(a.warmup):
            m(x, y, normalize=True)
        torch.cuda.synchronize()
        wall = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            d = m(x, y, normalize=True).cpu()
            wall.append(time.perf_counter() - t0)
        ev = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            m(x, y, normalize=True)
            e1.record()
            torch.cuda.synchronize()
            ev.append(e0.elapsed_time(e1))
        gf = conv_gflop(net, a.height, a.width) * 2 * a.batch
        res[net] = {"wall_ms_median": round(1e3 * float(np.median(wall)), 3), "wall_ms_min": round(1e3 * min(wall), 3),
                    "gpu_ms_median": round(float(np.median(ev)), 3), "gpu_ms_min": round(min(ev), 3),
                    "pairs_per_s": round(a.batch / float(np.median(wall)), 2),
                    "conv_gflop_per_image": round(conv_gflop(net, a.height, a.width), 1),
                    "conv_tflops_at_gpu_median": round(gf / float(np.median(ev)), 1),
                    "scores": [round(v, 6) for v in d.tolist()]}
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
