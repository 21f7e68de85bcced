"""Motion search and residual timing (fdn_hip.motion): one case per process, --what search | residual, --data u8 | u10 | u8in10, --radius R,
on B frames of h x w (each frame but the first matched against the one before it, the first against a frame handed in: B frame pairs).
  u8      8-bit frames: the search keeps four samples to a dword (v_sad_u8);
  u10     10-bit frames: two samples to a dword (v_sad_u16);
  u8in10  the codes of u8 stored in the 10-bit container: the arithmetic of u8 on the path of u10, which is what says whether the packed-
          byte path earns its place.
After a warm-up, `--reps` windows timed with HIP events around `--inner` back-to-back enqueues of the one entry point (outputs allocated
once; every repetition reads the same frames, which fit the Infinity Cache: the inputs are warm).  The figure is ms per frame pair: the
window over inner * B.  Next to it the share of one frame's forward (--forward-ms, README.md: 277 ms per 8 frames of 720 x 1280) and, for
the residual, the luma bytes of its four planes, their time at --hbm-gbs and the ratio of the measured time to that floor.  Prints one
JSON line; --out merges it into that file under the key <what>_<data>_r<R>_run<N>, so every case can run as a process of its own, each
under its own time limit, and alternated to show the run-to-run spread (--run N):

    for n in 1 2 3; do for d in u8 u8in10 u10; do for r in 8 16; do timeout 300 python tools/bench_motion.py --what search --data $d \\
        --radius $r --run $n --out profiles/motion_bench.json || break 3; done; done; done
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fdn-tip2025_amd"))
from fdn_hip import motion, stream  # noqa: E402
from fdn_hip.harness import VideoFormat  # noqa: E402


def stream_of(B, h, w, ten_bit_codes, seed):
    """B + 1 luma planes of one smoothed random texture drifting by (1, -2) pixels a frame, plus noise of +-2 codes: int64 [B+1,h,w]"""
    g = torch.Generator().manual_seed(seed)
    top = 1023 if ten_bit_codes else 255
    m = 2 * B + 2
    big = torch.randint(0, top + 1, (h + 2 * m, w + 2 * m), generator=g)
    big = (2 * big + big.roll(1, 0) + big.roll(1, 1)) // 4
    out = [big[m - t:m - t + h, m + 2 * t:m + 2 * t + w] + torch.randint(-2, 3, (h, w), generator=g) for t in range(B + 1)]
    return torch.stack(out).clamp_(0, top)


def frames_of(luma, dtype):
    B, h, w = luma.shape
    chroma = torch.full((B, h * w // 2), 128 if dtype == torch.uint8 else 512, dtype=torch.int64)
    f = torch.cat([luma.reshape(B, -1), chroma], dim=1)
    return (f.to(torch.uint8) if dtype == torch.uint8 else f.to(torch.int16)).to("cuda:0").contiguous()


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
    ap.add_argument("--what", choices=("search", "residual"), required=True)
    ap.add_argument("--data", choices=("u8", "u10", "u8in10"), required=True)
    ap.add_argument("--radius", type=int, default=8)
    ap.add_argument("--frames", type=int, default=8, help="B: frame pairs per call")
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=5, help="enqueues per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--run", type=int, default=1, help="which of the alternated runs this is (part of the key in --out)")
    ap.add_argument("--hbm-gbs", type=float, default=4000.0, help="the HBM rate the residual's floor is stated against, GB/s")
    ap.add_argument("--forward-ms", type=float, default=277.0 / 8, help="one frame's forward, ms (README.md: 277 ms per 8 frames)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, h, w, R = a.frames, a.height, a.width, a.radius
    ten = a.data != "u8"
    fmt = VideoFormat("yuv420p10le" if ten else "yuv420p")
    luma = stream_of(B, h, w, a.data == "u10", 7)
    guide = frames_of(luma, torch.int16 if ten else torch.uint8)
    noisy = frames_of((luma + torch.randint(-3, 4, luma.shape, generator=torch.Generator().manual_seed(8))).clamp_(0, 1023 if a.data == "u10" else 255),
                      torch.int16 if ten else torch.uint8)
    mv, sad, s_stats = motion.search(guide[1:], guide[:1], h, w, fmt, radius=R)
    r_stats = motion.residual(noisy[1:], noisy[:1], guide[1:], guide[:1], mv, h, w, fmt)
    torch.cuda.synchronize()
    l = motion.lib()
    p = lambda t: t.data_ptr()  # noqa: E731

    def search():
        l.fdn_motion_search(p(guide[1:]), p(guide[:1]), p(mv), p(sad), p(s_stats), B, h, w, fmt.bits, R, stream())

    def residual():
        l.fdn_motion_residual(p(noisy[1:]), p(noisy[:1]), p(guide[1:]), p(guide[:1]), p(mv), p(r_stats), B, h, w, fmt.bits, stream())
    launch = search if a.what == "search" else residual
    want = (s_stats if a.what == "search" else r_stats).clone()
    for _ in range(a.warmup):
        launch()
    torch.cuda.synchronize()
    assert torch.equal(s_stats if a.what == "search" else r_stats, want)          # the launches timed give what the module gave
    gpu = [v / B for v in events(launch, a.reps, a.inner)]
    found = s_stats.cpu().tolist()
    r = {"what": a.what, "data": a.data, "radius": R, "run": a.run, "frames": B, "height": h, "width": w, "reps": a.reps, "inner": a.inner,
         "ms_per_pair_median": round(gpu[0], 5), "ms_per_pair_min": round(gpu[1], 5), "ms_per_pair_max": round(gpu[2], 5),
         "forward_ms_per_frame": round(a.forward_ms, 3), "share_of_one_forward": round(gpu[0] / a.forward_ms, 5),
         "moving_blocks_share": round(sum(x[3] for x in found) / (B * mv.shape[1] * mv.shape[2]), 3),
         "device": torch.cuda.get_device_name(0)}
    if a.what == "residual":
        nbytes = 4 * h * w * (2 if ten else 1)                                    # the luma of two frames of each stream, once
        floor = nbytes / (a.hbm_gbs * 1e9) * 1e3
        r.update(bytes_per_pair=nbytes, hbm_gbs=a.hbm_gbs, floor_ms=round(floor, 5), times_floor=round(gpu[0] / floor, 1))
    print(json.dumps(r))
    if a.out:
        have = {}
        if os.path.isfile(a.out):
            with open(a.out) as f:
                have = json.load(f)
        have[f"{a.what}_{a.data}_r{R}_run{a.run}"] = r
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(dict(sorted(have.items())), indent=1) + "\n")


if __name__ == "__main__":
    main()
