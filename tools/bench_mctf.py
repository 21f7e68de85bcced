"""Temporal denoiser timing (fdn_hip.mctf): one case per process, --what blend | step, on B frames of h x w.
  blend   fdn_mctf_blend alone: B launches, frame i filtered against the output of frame i - 1, frame 0 against a frame handed in; the
          vectors come from one search beforehand;
  step    TemporalDenoiser.step on a stream that already has a frame before it: postprocess_yuv420 + one batched search + the blend, with
          the allocations and the two clones step makes.
The frames are one smoothed random R'G'B' texture drifting by (1, -2) pixels a frame plus noise, so the search finds vectors and the blend
takes its filtering path (asserted: no frame is a scene cut, and the weights are mostly above 0).  After a warm-up, `--reps` windows timed
with HIP events around `--inner` back-to-back calls (every repetition reads the same frames, which fit the Infinity Cache: the inputs are
warm).  The figure is ms per frame: the window over inner * B.  Next to it two yardsticks: the time of moving the blend's compulsory bytes
once at --hbm-gbs (36 B per pixel: cur read, the predecessor read, out written; fp32, three channels each), with the ratio of the measured
time to that floor, and the share of one frame's forward (--forward-ms, README.md: 277.8 ms per 8 frames of 720 x 1280).  Prints one JSON
line; --out merges it into that file under the key <what>_run<N>, so every case can run as a process of its own, each under its own time
limit, and alternated to show the run-to-run spread (--run N):

    for n in 1 2 3; do for k in blend step; do timeout 300 python tools/bench_mctf.py --what $k --run $n --out profiles/mctf_bench.json \\
        || break 2; done; done
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fdn-tip2025_amd"))
from fdn_hip import mctf, motion, stream  # noqa: E402
from fdn_hip.harness import VideoFormat, postprocess_yuv420  # noqa: E402


def stream_of(B, h, w, sigma, seed):
    """B + 1 fp32 frames [B+1,3,h,w] in [0, 1]: one smoothed random texture drifting by (1, -2) pixels a frame, plus Gaussian noise"""
    g = torch.Generator().manual_seed(seed)
    m = 2 * B + 2
    big = torch.rand((3, h + 2 * m, w + 2 * m), generator=g)
    for _ in range(2):
        big = (2 * big + big.roll(1, 1) + big.roll(1, 2)) / 4
    out = [big[:, m - t:m - t + h, m + 2 * t:m + 2 * t + w] + sigma * torch.randn((3, h, w), generator=g) for t in range(B + 1)]
    return torch.stack(out).clamp_(0, 1).to("cuda:0").contiguous()


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
    ap.add_argument("--what", choices=("blend", "step"), required=True)
    ap.add_argument("--frames", type=int, default=8, help="B: frames per call")
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--sigma", type=float, default=0.03, help="noise added to every frame")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=5, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--run", type=int, default=1, help="which of the alternated runs this is (part of the key in --out)")
    ap.add_argument("--hbm-gbs", type=float, default=4000.0, help="the HBM rate the blend's floor is stated against, GB/s")
    ap.add_argument("--forward-ms", type=float, default=277.8 / 8, help="one frame's forward, ms (README.md: 277.8 ms per 8 frames)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, h, w = a.frames, a.height, a.width
    fmt = VideoFormat("yuv420p")
    frames = stream_of(B, h, w, a.sigma, 7)
    cur, first = frames[1:], frames[0].contiguous()
    d = mctf.TemporalDenoiser(h, w, fmt, device="cuda:0")
    guide = postprocess_yuv420(frames, h, w, fmt)
    mv, _, stats = motion.search(guide[1:], guide[:1], h, w, fmt, radius=d.radius)
    out, k = mctf.blend(cur, first, mv, stats, h, w, d.strength, d.threshold, d.cut_limit, kmap=True)
    torch.cuda.synchronize()
    assert int(stats[:, 0].max()) <= d.cut_limit and float((k > 0).float().mean()) > 0.5      # the filtering path, not the bypass
    mean_k = float(k.mean())
    l, inv = mctf.lib(), mctf.inv_threshold(d.threshold)
    p = lambda t: t.data_ptr()  # noqa: E731

    def blend():
        l.fdn_mctf_blend(p(cur), p(first), p(mv), p(stats), p(out), None, B, h, w, h, w, d.strength, inv, d.cut_limit, stream())

    def step():
        d._guide, d._prev = guide[:1], first                                        # every call continues the same stream
        return d.step(cur)
    want = out.clone()
    if a.what == "blend":
        launch = blend
    else:
        launch = step
        assert torch.equal(step().view(torch.int32), want.view(torch.int32))       # step is post + search + this blend
    for _ in range(a.warmup):
        launch()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))              # the launches timed give what the module gave
    gpu = [v / B for v in events(launch, a.reps, a.inner)]
    nbytes = 36 * h * w                                                             # cur, the predecessor and out: 3 x fp32 each per pixel
    floor = nbytes / (a.hbm_gbs * 1e9) * 1e3
    r = {"what": a.what, "run": a.run, "frames": B, "height": h, "width": w, "reps": a.reps, "inner": a.inner, "sigma": a.sigma,
         "ms_per_frame_median": round(gpu[0], 5), "ms_per_frame_min": round(gpu[1], 5), "ms_per_frame_max": round(gpu[2], 5),
         "blend_bytes_per_frame": nbytes, "hbm_gbs": a.hbm_gbs, "blend_floor_ms": round(floor, 5), "times_blend_floor": round(gpu[0] / floor, 1),
         "forward_ms_per_frame": round(a.forward_ms, 3), "share_of_one_forward": round(gpu[0] / a.forward_ms, 5), "mean_k": round(mean_k, 3),
         "device": torch.cuda.get_device_name(0)}
    print(json.dumps(r))
    if a.out:
        have = {}
        if os.path.isfile(a.out):
            with open(a.out) as f:
                have = json.load(f)
        have[f"{a.what}_run{a.run}"] = r
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(dict(sorted(have.items())), indent=1) + "\n")


if __name__ == "__main__":
    main()
