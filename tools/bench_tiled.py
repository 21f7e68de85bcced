"""Tiled inference timing: one synthetic uint8 frame (default 3000 x 4000, 20 tiles of 736 x 1280 under tile="auto") through
fdn_hip.harness.enhance_u8 with the tamed synthetic weights of the test suite (the time does not depend on the values), wall clock around
a synchronised call and torch.cuda.max_memory_allocated; and the two uint8 <-> tile kernels of ABI 21 against the four-call compositions
they replace (fdn_pre_u8 + fdn_tiles_gather, fdn_tiles_merge + fdn_post_u8) at the same size, HIP events around the launches; and the
feathered uint8 merge (fdn_tiles_merge_w_u8) beside the averaging one.  The shader clock is sampled while the frame runs
(bench.GpuSensors).  Prints one JSON line; --out writes it too.

    python tools/bench_tiled.py --reps 3 --out profiles/tiled_bench.json
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "fdn-tip2025_amd")):
    sys.path.insert(0, p)
import fdn_hip  # noqa: E402
from bench import GpuSensors  # noqa: E402
from common import fdn_weights, lpnet_weights  # noqa: E402
from fdn_hip import harness, tiling  # noqa: E402


def gpu_ms(fn, reps):
    ev = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ev.append(e0.elapsed_time(e1))
    return {"gpu_ms_median": round(float(np.median(ev)), 3), "gpu_ms_min": round(min(ev), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=3000)
    ap.add_argument("--width", type=int, default=4000)
    ap.add_argument("--batch", type=int, default=8, help="tiles per forward")
    ap.add_argument("--overlap", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from basicsr.models.archs.FDN_arch import FDN
    from basicsr.models.archs.LPNet_arch import I_predict_net
    dev = torch.device("cuda:0")
    net, lp = FDN().eval(), I_predict_net().eval()
    net.load_state_dict(fdn_weights(tame=0.03), strict=True)
    lp.load_state_dict(lpnet_weights(), strict=True)
    net, lp = net.to(dev), lp.to(dev)
    h, w = a.height, a.width
    img = (torch.rand(h, w, 3, generator=torch.Generator().manual_seed(7)) * 96).to(torch.uint8).to(dev)
    crop = harness.resolve_tile("auto", h, w)
    if crop is None:
        raise SystemExit(f"a {h}x{w} frame is not tiled under tile='auto'")
    n_tiles = len(tiling.tile_origins(h, w, *tiling.effective_crop(h, w, *crop), a.overlap))
    res = {"what": "fdn_hip.harness.enhance_u8(tile='auto')", "height": h, "width": w, "tile": list(crop), "tiles": n_tiles,
           "tiles_per_forward": a.batch, "overlap": a.overlap, "reps": a.reps}

    def frame():
        return harness.enhance_u8(net, lp, img, bgr=False, tile="auto", overlap=a.overlap, batch=a.batch)
    for _ in range(a.warmup):
        frame()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    wall = []
    with GpuSensors(0) as sensors:
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out = frame()
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
    res["frame"] = {"wall_ms_median": round(1e3 * float(np.median(wall)), 1), "wall_ms_min": round(1e3 * min(wall), 1),
                    "ms_per_tile": round(1e3 * float(np.median(wall)) / n_tiles, 2),
                    "max_memory_allocated_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 3),
                    "output_mean": round(float(out.float().mean()), 3)}
    res["sensors"] = sensors.summary()
    del out
    torch.cuda.empty_cache()

    # the two kernels against what they replace, on the same frame and origins
    tiles, ij = tiling.split_u8(img, *crop, bgr=False, overlap=a.overlap)
    outs = torch.rand(tiles.shape, device=dev) * 1.4 - 0.2

    def four_call_in():
        x = torch.empty((1, 3, h, w), device=dev, dtype=torch.float32)                  # fdn_pre_u8 with H = h, W = w: no padding
        fdn_hip.check(fdn_hip.lib().fdn_pre_u8(ctypes.c_void_p(img.data_ptr()), ctypes.c_void_p(x.data_ptr()), 1, h, w, h, w, 0, fdn_hip.stream()),
                      "fdn_pre_u8")
        return tiling.split(x, tiles.shape[2], tiles.shape[3], a.overlap)

    def four_call_out():
        return harness.postprocess(tiling.merge(outs, ij, h, w), h, w, bgr=False)
    same_in = torch.equal(four_call_in()[0], tiles)
    same_out = torch.equal(four_call_out()[0], tiling.merge_u8(outs, ij, h, w, bgr=False))
    res["gather"] = {"fdn_tiles_gather_u8": gpu_ms(lambda: tiling.split_u8(img, *crop, bgr=False, overlap=a.overlap), a.kernel_reps),
                     "fdn_pre_u8 + fdn_tiles_gather": gpu_ms(four_call_in, a.kernel_reps), "bit_equal": same_in}
    res["merge"] = {"fdn_tiles_merge_u8": gpu_ms(lambda: tiling.merge_u8(outs, ij, h, w, bgr=False), a.kernel_reps),
                    "fdn_tiles_merge + fdn_post_u8": gpu_ms(four_call_out, a.kernel_reps), "bit_equal": same_out}

    # the feathered merge beside the average: the launch alone (weights already on the device), and tiling.merge_u8(blend="feather") as the
    # route calls it, which builds the weight vectors on the host and copies them for every frame
    idx = ij.cpu().tolist()
    wy, wx = (t.to(dev).contiguous() for t in tiling.feather_weights(idx, tiles.shape[2], tiles.shape[3]))
    out_w = torch.empty((h, w, 3), device=dev, dtype=torch.uint8)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def feather_launch():
        fdn_hip.check(fdn_hip.lib().fdn_tiles_merge_w_u8(ptr(outs), ptr(out_w), ptr(ij), ptr(wy), ptr(wx), len(idx), h, w, tiles.shape[2],
                                                         tiles.shape[3], 0, fdn_hip.stream()), "fdn_tiles_merge_w_u8")
    out_a = torch.empty_like(out_w)

    def average_launch():
        fdn_hip.check(fdn_hip.lib().fdn_tiles_merge_u8(ptr(outs), ptr(out_a), ptr(ij), len(idx), h, w, tiles.shape[2], tiles.shape[3], 0,
                                                       fdn_hip.stream()), "fdn_tiles_merge_u8")
    feather_launch()
    same_w = torch.equal(out_w, harness.postprocess(tiling.merge(outs, ij, h, w, blend="feather"), h, w, bgr=False)[0])
    res["merge_feather"] = {"fdn_tiles_merge_w_u8 (launch)": gpu_ms(feather_launch, a.kernel_reps),
                            "fdn_tiles_merge_u8 (launch)": gpu_ms(average_launch, a.kernel_reps),
                            "tiling.merge_u8(blend='feather') with host weights": gpu_ms(lambda: tiling.merge_u8(outs, ij, h, w, bgr=False, blend="feather"),
                                                                                         a.kernel_reps),
                            "bytes_differing_from_average": int((out_w != tiling.merge_u8(outs, ij, h, w, bgr=False)).sum()),
                            "bit_equal_to_fdn_tiles_merge_w + fdn_post_u8": same_w}
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
