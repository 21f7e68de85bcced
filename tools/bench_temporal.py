"""Timing of the ratio filter across frames beside the forward it sits in: fdn_hip.temporal.RatioFilter.step (fdn_luma_hist +
fdn_ratio_smooth, the scratch it keeps and the count of cuts) on one batch of frames, 8 and 10 bit, at 720p and 1080p, and the
LPNet -> FDN forward of the same batch in the same process.  HIP events around windows of `--launches` back-to-back steps after a warm-up,
the median and the least window reported per step with the luma bytes a step has to read over the median; the forward as the median of
`--forward-runs` single runs.  Prints one JSON line; --out writes it too.

    python tools/bench_temporal.py --out profiles/temporal_bench.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fdn-tip2025_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from fdn_hip import harness  # noqa: E402
from fdn_hip.temporal import RatioFilter  # noqa: E402


def size_arg(s):
    w, h = (int(v) for v in s.lower().split("x"))
    return h, w


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=size_arg, nargs="+", default=[(720, 1280), (1080, 1920)], metavar="WxH")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--launches", type=int, default=200, help="steps per timed window")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--forward-runs", type=int, default=3, help="timed forwards per size, after one warm-up (0: skip the forward)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_temporal.py needs a ROCm GPU")
    from basicsr.models.archs.FDN_arch import FDN
    from basicsr.models.archs.LPNet_arch import I_predict_net
    from common import fdn_weights, lpnet_weights
    dev = torch.device("cuda:0")
    net, lp = FDN().eval(), I_predict_net().eval()
    net.load_state_dict(fdn_weights(tame=0.03), strict=True)
    lp.load_state_dict(lpnet_weights(), strict=True)
    net, lp = net.to(dev), lp.to(dev)
    B = a.batch
    g = torch.Generator().manual_seed(5)
    out = {"what": "RatioFilter.step per call (two launches, HIP events around windows of back-to-back steps) beside the LPNet -> FDN forward "
                   "of the same batch (eager, one run per HIP-event pair)", "batch": B, "launches_per_window": a.launches, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0), "sizes": {}}
    for h, w in a.sizes:
        entry = {}
        for pix in ("yuv420p", "yuv420p10le"):
            fmt = harness.VideoFormat(pix, "bt709", False, "left")
            n = fmt.frame_samples(h, w)
            s = 2 ** (fmt.bits - 8)
            # dim, noisy frames: luma in the lowest fifth of the range, so the increments crowd into few bins as low-light footage does
            frames = torch.randint(16 * s, 60 * s, (B, n), generator=g).to(fmt.dtype).to(dev)
            ratio = torch.rand(B, 1, generator=g).to(dev) * 0.5 + 0.05
            f = RatioFilter(h, w, fmt.bits, 0.25, device=dev)
            step = lambda: f.step(frames, ratio)  # noqa: E731
            timed(step, 20)
            windows = [timed(step, a.launches) for _ in range(a.rounds)]
            med, nbytes = float(np.median(windows)), B * h * w * fmt.sample_bytes
            entry[pix] = {"step_ms_median": round(med, 4), "step_ms_min": round(min(windows), 4), "step_ms_max": round(max(windows), 4),
                          "luma_bytes": nbytes, "GB_per_s_at_median": round(nbytes / med / 1e6, 1)}
            if a.forward_runs and pix == "yuv420p":
                with torch.no_grad():
                    x = harness.preprocess_yuv420(frames, h, w, fmt)[0]
                    fwd = lambda: net(x, ratio_i=lp(x), device=x.device)[0]  # noqa: E731
                    timed(fwd, 1)
                    runs = [timed(fwd, 1) for _ in range(a.forward_runs)]
                entry["forward_ms_median"] = round(float(np.median(runs)), 2)
                entry["forward_ms_min"] = round(min(runs), 2)
                del x
                torch.cuda.empty_cache()
        if "forward_ms_median" in entry:
            for pix in ("yuv420p", "yuv420p10le"):
                entry[pix]["share_of_forward"] = round(entry[pix]["step_ms_median"] / entry["forward_ms_median"], 6)
        out["sizes"][f"{w}x{h}"] = entry
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
