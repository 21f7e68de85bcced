"""Multi-scale SSIM (Wang, Simoncelli, Bovik 2003) per pair of a restored image and its ground truth, on the HIP path (fdn_hip.msssim):
contrast and structure over five octaves, luminance only at the coarsest, 1 for equal images.  --mode rgb (default) scores R, G and B on
their own and prints their mean; --mode gray scores the one plane 0.299 R + 0.587 G + 0.114 B (kept as the integer 299 R + 587 G + 114 B;
not the Y of bgr2ycbcr, so tools that score that Y differ slightly).  The pyramid is Wang's (2 x 2 means, the last row / column counted
twice at odd sizes), the window the 11 x 11 Gaussian of sigma 1.5 over 'valid' positions.  Five scales need images of at least 161x161:
a smaller one is refused, no scale is dropped.  Beside the score the five per-level means are printed (contrast-structure of levels
0 .. 3, the full SSIM of level 4), unclamped: a negative one makes the score 0.  The globs are sorted and paired by index; unequal counts
and unequal sizes within a pair are errors.  Images of equal size are scored as one batch, with one device-to-host copy per batch.  Needs
a ROCm GPU and the built libfdn_msssim.so; there is no CPU fallback.  Images must be 8-bit RGB.

    python calculate_ms_ssim.py --gt 'lolblur/test/high_sharp_scaled/*/*' --restored 'results/lolblur/*/*' --csv ms_ssim.csv

--save-map DIR writes, per pair, the full-resolution (level 0) SSIM map l * cs as an 8-bit grey PNG, clipped to [0, 1]; for --mode rgb
the mean of the three channels' maps.
"""
import argparse
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from calculate_sharpness_metrics import decoded_groups, match_paths, write_map  # noqa: E402

LEVEL_KEYS = ("cs0", "cs1", "cs2", "cs3", "ss4")


def score(items, mode="rgb", batch=8, device="cuda:0", save_map=None, workers=4):
    """(restored, gt) paths -> per pair, in order, one dict of fdn_hip.msssim.ms_ssim_u8"""
    import torch
    from fdn_hip import msssim
    dev = torch.device(device)
    torch.cuda.set_device(dev)
    out = [None] * len(items)
    with ThreadPoolExecutor(max_workers=workers) as pool:
        for idx, cols in decoded_groups(items, batch, pool):
            rs, gt = (torch.from_numpy(c).to(dev) for c in cols)
            if save_map:
                res, (_, ss) = msssim.ms_ssim_maps_u8(gt, rs, mode=mode, bgr=False, with_scores=True)
                planes = 3 if mode == "rgb" else 1
                maps = ss[0].view(len(idx), planes, *ss[0].shape[1:]).cpu().numpy()
            else:
                res = msssim.ms_ssim_u8(gt, rs, mode=mode, bgr=False)
            for k, i in enumerate(idx):
                out[i] = res[k]
                if save_map:
                    m = maps[k][0] if mode == "gray" else (maps[k][0] + maps[k][1] + maps[k][2]) / 3
                    write_map(os.path.join(save_map, os.path.splitext(os.path.basename(items[i][0]))[0] + ".png"), m)
    return out


def ms_ssim_line(m):
    """the figures of one pair"""
    return f"MS-SSIM: {m['ms_ssim']:.6f} (levels " + " ".join(f"{v:.6f}" for v in m["levels"]) + ")"


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--restored", required=True, help="the restored images: a glob, sorted")
    ap.add_argument("--gt", required=True, help="ground-truth images: a glob, sorted and paired with --restored by index")
    ap.add_argument("--mode", choices=("rgb", "gray"), default="rgb", help="score R, G, B on their own and average (default), or the gray plane")
    ap.add_argument("--batch", type=int, default=8, help="images of equal size scored per launch")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--csv", default=None, help="file for one line per pair")
    ap.add_argument("--save-map", default=None, metavar="DIR", help="directory for the level-0 SSIM pictures, one 8-bit grey PNG per pair")
    a = ap.parse_args(argv)
    if a.batch < 1:
        ap.error("--batch must be >= 1")
    try:
        a.items = match_paths(a.restored, a.gt)
    except ValueError as e:
        ap.error(str(e))
    return a


def main(argv=None):
    a = parse_args(argv)
    from fdn_hip import FdnHipError
    try:
        res = score(a.items, a.mode, a.batch, a.device, a.save_map)
    except (FdnHipError, ValueError) as e:
        sys.exit(f"calculate_ms_ssim.py: {e}")
    n = len(res)
    for i, (it, m) in enumerate(zip(a.items, res)):
        basename = os.path.splitext(os.path.basename(it[0]))[0]
        print(f"{i+1:3d}: {basename:25}. \t{ms_ssim_line(m)}")
    print(f"Average: {ms_ssim_line({'ms_ssim': sum(m['ms_ssim'] for m in res) / n, 'levels': [sum(m['levels'][s] for m in res) / n for s in range(5)]})}")
    if a.csv:
        os.makedirs(os.path.dirname(a.csv) or ".", exist_ok=True)
        with open(a.csv, "w") as f:
            f.write("restored,gt,ms_ssim," + ",".join(LEVEL_KEYS) + (",ms_ssim_r,ms_ssim_g,ms_ssim_b" if a.mode == "rgb" else "") + "\n")
            for it, m in zip(a.items, res):
                tail = "," + ",".join(repr(v) for v in m["channels"]) if a.mode == "rgb" else ""
                f.write(f"{it[0]},{it[1]},{m['ms_ssim']!r}," + ",".join(repr(v) for v in m["levels"]) + tail + "\n")


if __name__ == "__main__":
    main()
