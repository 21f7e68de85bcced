"""Exposure fusion timing (fdn_hip.fusion): the weights, the pyramid on given weights, or the whole fuse (--what) of K renderings (--k) of
an h x w frame.  After a warm-up, `--reps` windows timed with HIP events around `--inner` back-to-back enqueues of the launches alone
(workspace and outputs allocated once; the figure is the window over `--inner`; every repetition reads the same buffers, which at the
default size fit the Infinity Cache: the inputs are warm).  Next to the times, the bytes the step must move at the least - its inputs
read once and its outputs written once, the pyramids kept on chip - the time that takes at --hbm-gbs, the ratio of the measured time to
that floor, the bytes the launches as built move (every level >= 1 of the pyramids written once and read by the next down, by its own
blend and by the blend of the level above), and for `fuse` the share of one frame's forward (--forward-ms, README.md: 277.8 ms per 8
frames of 720 x 1280) that fusing costs.  Prints one JSON line; --out merges it into that file under the key <what>_k<K>, so every case can
run as a process of its own, each under its own time limit:

    for k in 3 5; do for w in weights pyramid fuse; do timeout 300 python tools/bench_fusion.py --what $w --k $k --out profiles/fusion_bench.json || break 2; done; done
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fdn-tip2025_amd"))
from fdn_hip import fusion, ptr, stream  # noqa: E402

CASES = ("weights", "pyramid", "fuse")


def renderings(K, h, w, seed):
    """K renderings of one textured scene from dark to bright, fp32 [K,3,h,w], some samples outside [0, 1]"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    base = 0.45 + 0.2 * torch.sin(xx / 7.0) * torch.cos(yy / 9.0) + 0.1 * ((xx // 16 + yy // 12) % 2)
    scene = torch.stack([base * 0.9, base, base * 1.1])
    gains = torch.linspace(0.3, 1.9, K)
    return torch.stack([scene * a + 0.02 * torch.randn(3, h, w, generator=g) for a in gains]).contiguous()


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


def bytes_moved(what, K, h, w):
    """(least, as built): bytes of the step's inputs and outputs once, and of what its launches read and write"""
    hw = h * w
    upper = sum(a * b for a, b in fusion.dims(h, w)[1][1:])                       # samples of levels 1 .. L
    last = fusion.dims(h, w)[1][-1][0] * fusion.dims(h, w)[1][-1][1] if fusion.dims(h, w)[0] else 0
    w_least = w_built = 4 * (3 * K + K) * hw                                      # the neighbours of a pixel come from the caches
    # level 0: down reads 4 K planes, the blend reads them again and writes 3; levels >= 1: 4 K planes written, read by the next down
    # (but the last), by their own blend (4 K) and by the blend above (3 K); the collapse written and read (3 + 3, level 0: written)
    p_built = 4 * ((4 * K + 4 * K + 3) * hw + (4 * K + 4 * K + 3 * K + 6) * upper + 4 * K * (upper - last))
    p_least = 4 * (4 * K + 3) * hw
    if what == "weights":
        return w_least, w_built
    if what == "pyramid":
        return p_least, p_built
    return 4 * (3 * K + 3) * hw, w_built + p_built                                # an ideal fuse never writes the weights


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=CASES, required=True)
    ap.add_argument("--k", type=int, default=3, help="renderings")
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20, help="enqueues per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hbm-gbs", type=float, default=4000.0, help="the HBM rate the floor is stated against, GB/s")
    ap.add_argument("--forward-ms", type=float, default=277.8 / 8, help="one frame's forward, ms (README.md: 277.8 ms per 8 frames)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    K, h, w = a.k, a.height, a.width
    imgs = renderings(K, h, w, 7).to("cuda:0")
    l = fusion.lib()
    wts = torch.empty((K, h, w), dtype=torch.float32, device="cuda:0")
    out = torch.empty((3, h, w), dtype=torch.float32, device="cuda:0")
    nws = int(l.fdn_fusion_ws(K, h, w))
    work = torch.empty(max(nws // 4, 4), dtype=torch.float32, device="cuda:0")

    def weights():
        l.fdn_fuse_weights(ptr(imgs), ptr(wts), K, h, w, h, w, 1.0, 1.0, 1.0, stream())

    def pyramid():
        l.fdn_fuse_pyramid(ptr(imgs), ptr(wts), ptr(out), ptr(work), K, h, w, h, w, stream())
    launch = {"weights": weights, "pyramid": pyramid, "fuse": lambda: (weights(), pyramid())}[a.what]
    weights()                                                                     # the pyramid alone runs on real weights
    for _ in range(a.warmup):
        launch()
    torch.cuda.synchronize()
    assert torch.equal(fusion.fuse(imgs, h, w), out) or a.what == "weights"       # the launches timed are the module's
    gpu = events(launch, a.reps, a.inner)
    least, built = bytes_moved(a.what, K, h, w)
    floor = least / (a.hbm_gbs * 1e9) * 1e3
    r = {"what": a.what, "k": K, "height": h, "width": w, "levels": fusion.dims(h, w)[0], "reps": a.reps, "inner": a.inner,
         "gpu_ms_median": round(gpu[0], 4), "gpu_ms_min": round(gpu[1], 4), "gpu_ms_max": round(gpu[2], 4),
         "bytes_least": least, "bytes_as_built": built, "hbm_gbs": a.hbm_gbs, "floor_ms": round(floor, 4), "times_floor": round(gpu[0] / floor, 1),
         "device": torch.cuda.get_device_name(0)}
    if a.what == "fuse":
        r["forward_ms_per_frame"] = round(a.forward_ms, 3)
        r["share_of_one_forward"] = round(gpu[0] / a.forward_ms, 4)
    print(json.dumps(r))
    if a.out:
        have = {}
        if os.path.isfile(a.out):
            with open(a.out) as f:
                have = json.load(f)
        have[f"{a.what}_k{K}"] = r
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(dict(sorted(have.items())), indent=1) + "\n")


if __name__ == "__main__":
    main()
