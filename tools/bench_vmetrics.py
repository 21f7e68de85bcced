"""Timing of video evaluation from codec samples: what fdn_hip.video_metrics.VideoScore.update enqueues for one batch of frame pairs -
pair_stats (fdn_yuv420_pair_stats), ssim_y (fdn_yuv420_ssim_y) and fdn_luma_hist - 8 and 10 bit, at 720p and 1080p, and beside them in
the same process the route that existed before: fdn_ssim2d(replicate_no_crop=1) on the same luma as fp32 planes, frame by frame, with its
5 h w doubles of workspace per frame.  HIP events around windows of `--launches` back-to-back calls after a warm-up; the median and the
least window are reported per call, with the sample bytes a call has to read over the median.  These are CALL times: a window holds what
the Python wrappers do per call (two allocations in ssim_y, one in pair_stats) as well as the launches, and for a launch of some 10 us the
host's enqueue rate can be what is measured; the `*_raw` figures call the C entry points on buffers allocated once, so the two can be told
apart.  Prints one JSON line; --out writes it too.

    python tools/bench_vmetrics.py --out profiles/vmetrics_bench.json
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fdn-tip2025_amd")):
    sys.path.insert(0, p)
import fdn_hip  # noqa: E402
from fdn_hip import harness, metrics, video_metrics  # noqa: E402


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


def windows(fn, launches, rounds):
    timed(fn, 10)
    w = [timed(fn, launches) for _ in range(rounds)]
    return {"ms_median": round(float(np.median(w)), 4), "ms_min": round(min(w), 4), "ms_max": round(max(w), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=size_arg, nargs="+", default=[(720, 1280), (1080, 1920)], metavar="WxH")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--launches", type=int, default=200, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vmetrics.py needs a ROCm GPU")
    dev = torch.device("cuda:0")
    B = a.batch
    g = torch.Generator().manual_seed(5)
    out = {"what": "call times of one batch of frame pairs: pair_stats, ssim_y, fdn_luma_hist and the three together through the Python wrappers "
                   "(HIP events around windows of back-to-back calls; the wrappers' allocations are inside), the two C entry points on "
                   "buffers allocated once (*_raw), and fdn_ssim2d on fp32 luma planes frame by frame (the route before)", "batch": B,
           "launches_per_window": a.launches, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "sizes": {}}
    for h, w in a.sizes:
        entry = {}
        for pix in ("yuv420p", "yuv420p10le"):
            fmt = harness.VideoFormat(pix, "bt709", False, "left")
            n, top = fmt.frame_samples(h, w), 2 ** fmt.bits - 1
            ref = torch.randint(0, top + 1, (B, n), generator=g)
            dist = (ref + torch.randint(-3, 4, (B, n), generator=g)).clamp_(0, top)
            ref, dist = ref.to(fmt.dtype).to(dev), dist.to(fmt.dtype).to(dev)
            hist = torch.empty((B, 256), dtype=torch.int32, device=dev)

            def luma_hist():
                fdn_hip.check(fdn_hip.lib().fdn_luma_hist(ctypes.c_void_p(ref.data_ptr()), ctypes.c_void_p(hist.data_ptr()), B, h, w, fmt.bits,
                                                          fdn_hip.stream()), "fdn_luma_hist")

            def all_three():
                video_metrics.pair_stats(dist, ref, h, w, fmt)
                video_metrics.ssim_y(dist, ref, h, w, fmt)
                luma_hist()
            stats = torch.empty((B, 5), dtype=torch.int64, device=dev)
            part = torch.empty(int(fdn_hip.lib().fdn_yuv420_ssim_y_ws(B, h, w)), dtype=torch.float64, device=dev)
            score = torch.empty(B, dtype=torch.float64, device=dev)
            taps = np.ascontiguousarray(metrics.ssim3d_taps(), dtype=np.float64)
            ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

            def stats_raw():
                fdn_hip.check(fdn_hip.lib().fdn_yuv420_pair_stats(ptr(dist), ptr(ref), ptr(stats), B, h, w, fmt.layout, fmt.bits, fdn_hip.stream()),
                              "fdn_yuv420_pair_stats")

            def ssim_raw():
                fdn_hip.check(fdn_hip.lib().fdn_yuv420_ssim_y(ptr(dist), ptr(ref), ptr(score), ptr(part), ctypes.c_void_p(taps.ctypes.data), B, h, w,
                                                              fmt.bits, fdn_hip.stream()), "fdn_yuv420_ssim_y")
            e = {"pair_stats": windows(lambda: video_metrics.pair_stats(dist, ref, h, w, fmt), a.launches, a.rounds),
                 "ssim_y": windows(lambda: video_metrics.ssim_y(dist, ref, h, w, fmt), a.launches, a.rounds),
                 "luma_hist": windows(luma_hist, a.launches, a.rounds),
                 "all": windows(all_three, a.launches, a.rounds),
                 "pair_stats_raw": windows(stats_raw, a.launches, a.rounds), "ssim_y_raw": windows(ssim_raw, a.launches, a.rounds)}
            # bytes a call reads: both streams whole for the stats, both luma planes for SSIM, one luma plane for the histogram
            nb = B * h * w * fmt.sample_bytes
            e["bytes_read"] = 3 * nb + 2 * nb + nb
            e["bytes_per_pixel"] = round(e["bytes_read"] / (B * h * w), 2)
            e["GB_per_s_at_median"] = round(e["bytes_read"] / e["all"]["ms_median"] / 1e6, 1)
            # the route before: float32 luma planes (made once, not timed), fdn_ssim2d per frame with 5 h w doubles of workspace
            ya = dist[:, :h * w].to(torch.int32).bitwise_and_(0xFFFF).clamp_(0, top).to(torch.float32).reshape(B, 1, h, w).contiguous()
            yb = ref[:, :h * w].to(torch.int32).bitwise_and_(0xFFFF).clamp_(0, top).to(torch.float32).reshape(B, 1, h, w).contiguous()
            ws = torch.empty(5 * h * w, dtype=torch.float64, device=dev)
            acc = torch.zeros(B, dtype=torch.float64, device=dev)

            def ssim2d():
                acc.zero_()
                for b in range(B):
                    fdn_hip.check(fdn_hip.lib().fdn_ssim2d(ctypes.c_void_p(ya[b].data_ptr()), ctypes.c_void_p(yb[b].data_ptr()), 1, h, w,
                                                           ctypes.c_float(float(top)), 1, ctypes.c_void_p(ws.data_ptr()),
                                                           ctypes.c_void_p(acc[b:].data_ptr()), fdn_hip.stream()), "fdn_ssim2d")
            e["fdn_ssim2d_per_frame_route"] = windows(ssim2d, max(1, a.launches // 5), a.rounds)
            e["fdn_ssim2d_workspace_bytes"] = 5 * h * w * 8
            e["ssim_y_workspace_bytes"] = int(fdn_hip.lib().fdn_yuv420_ssim_y_ws(B, h, w)) * 8
            fused = video_metrics.ssim_y(dist, ref, h, w, fmt)
            ssim2d()
            e["max_abs_diff_of_the_two_routes"] = float((fused - acc / (h * w)).abs().max())
            entry[pix] = e
            del ya, yb, ws
            torch.cuda.empty_cache()
        out["sizes"][f"{w}x{h}"] = entry
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
