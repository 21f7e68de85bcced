"""The three figures that tell a soft picture from a sharp one, on the HIP path (fdn_hip.sharpness): with --gt, per pair of a restored
image and its ground truth, the edge error (the reference's EdgeLoss as an evaluation figure; 0.001 for equal images), GMSD (gradient
magnitude similarity deviation; 0 for equal images) and the mean gradient magnitude of both images with their ratio, restored over ground
truth - below 1 the restored image is softer than the truth, above 1 it was over-sharpened or is noisy.  Without --gt only the restored
images' own mean gradient is printed, which needs no ground truth, so that real footage can be scored.  The globs are sorted and paired
by index; unequal counts and unequal sizes within a pair are errors.  Images of equal size are scored as one batch, with one device-to-host
copy per batch.  Needs a ROCm GPU and the built libfdn_sharpness.so; there is no CPU fallback.  Images must be 8-bit RGB.

    python calculate_sharpness_metrics.py --gt 'lolblur/test/high_sharp_scaled/*/*' --restored 'results/lolblur/*/*' --csv sharpness.csv

--save-gms-map DIR writes, per pair, the gradient magnitude similarity q of every point of GMSD's half-resolution grid (1 where the two
gradients agree) as an 8-bit grey PNG.
"""
import argparse
import glob
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from calculate_lpips import group_pairs, pair_paths, read_rgb8  # noqa: E402
from calculate_psnr_ssim import image_shape  # noqa: E402


def match_paths(restored_glob, gt_glob=None):
    """the sorted globs paired by index -> [(restored,)] or [(restored, gt)]"""
    if gt_glob is not None:
        return [(r, g) for g, r in pair_paths(gt_glob, restored_glob)]
    rs = sorted(glob.glob(restored_glob))
    if not rs:
        raise ValueError(f"no restored images match {restored_glob!r}")
    return [(r,) for r in rs]


def decoded_groups(items, batch, pool):
    """tuples of 1 or 2 paths -> (indices, [images [n][h][w][3] per position]) per group of tuples of one size, at most `batch` each;
    the group handed out and the next one, decoding on `pool` meanwhile, are all that is in host memory"""
    shapes = [[image_shape(p) for p in it] for it in items]
    groups = group_pairs([(s[-1], s[0]) for s in shapes], batch)
    width = len(items[0])

    def submit(idx):
        return [[pool.submit(read_rgb8, items[i][k]) for i in idx] for k in range(width)]
    ahead = submit(groups[0])
    for n, idx in enumerate(groups):
        now, ahead = ahead, submit(groups[n + 1]) if n + 1 < len(groups) else None
        yield idx, [np.stack([f.result() for f in col]) for col in now]


def score(items, batch=8, device="cuda:0", save_map=None, workers=4):
    """-> per tuple of paths, in order: one dict of fdn_hip.sharpness.sharpness_metrics, or {"grad_restored": ...} for a tuple without
    a ground truth"""
    import torch
    from fdn_hip import sharpness
    dev = torch.device(device)
    torch.cuda.set_device(dev)
    out = [None] * len(items)
    with ThreadPoolExecutor(max_workers=workers) as pool:
        for idx, cols in decoded_groups(items, batch, pool):
            t = [torch.from_numpy(c).to(dev) for c in cols]
            if len(t) == 1:
                res = [{"grad_restored": m} for m in sharpness.mean_gradient_u8(t[0], bgr=False)]
            else:
                res = sharpness.sharpness_metrics(t[1], t[0], bgr=False, want_gms_map=bool(save_map))
                if save_map:
                    res, maps = res[0], res[1].cpu().numpy()
            for k, i in enumerate(idx):
                out[i] = res[k]
                if save_map and len(t) == 2:
                    write_map(os.path.join(save_map, os.path.splitext(os.path.basename(items[i][0]))[0] + ".png"), maps[k])
    return out


def map_bytes(q):
    """q of every grid point, in [0, 1] -> the 8-bit picture"""
    return np.rint(np.clip(q.astype(np.float64), 0.0, 1.0) * 255.0).astype(np.uint8)


def write_map(path, q):
    from PIL import Image
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    Image.fromarray(map_bytes(q), mode="L").save(path)


def sharpness_line(m):
    """the figures of one pair, as printed here and by validate_fdn.py --sharpness"""
    return f"edge: {m['edge']:.6f}, GMSD: {m['gmsd']:.6f}, grad ratio: {m['grad_ratio']:.6f}"


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--restored", required=True, help="the restored images: a glob, sorted")
    ap.add_argument("--gt", default=None, help="ground-truth images: a glob, sorted and paired with --restored by index; without it the mean gradient only")
    ap.add_argument("--batch", type=int, default=8, help="images of equal size scored per launch")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--csv", default=None, help="file for one line per image")
    ap.add_argument("--save-gms-map", default=None, metavar="DIR", help="directory for the similarity pictures, one 8-bit grey PNG per pair")
    a = ap.parse_args(argv)
    if a.batch < 1:
        ap.error("--batch must be >= 1")
    if a.save_gms_map and not a.gt:
        ap.error("--save-gms-map needs --gt: the similarity is of a pair")
    try:
        a.items = match_paths(a.restored, a.gt)
    except ValueError as e:
        ap.error(str(e))
    return a


def main(argv=None):
    a = parse_args(argv)
    from fdn_hip import FdnHipError
    try:
        res = score(a.items, a.batch, a.device, a.save_gms_map)
    except (FdnHipError, ValueError) as e:
        sys.exit(f"calculate_sharpness_metrics.py: {e}")
    n = len(res)
    for i, (it, m) in enumerate(zip(a.items, res)):
        basename = os.path.splitext(os.path.basename(it[0]))[0]
        line = f"{sharpness_line(m)} (gt {m['grad_gt']:.6f}, restored {m['grad_restored']:.6f})" if a.gt else f"grad: {m['grad_restored']:.6f}"
        print(f"{i+1:3d}: {basename:25}. \t{line}")
    if a.gt:
        print(f"Average: {sharpness_line({k: sum(m[k] for m in res) / n for k in ('edge', 'gmsd', 'grad_ratio')})}")
    else:
        print(f"Average: grad: {sum(m['grad_restored'] for m in res) / n:.6f}")
    if a.csv:
        os.makedirs(os.path.dirname(a.csv) or ".", exist_ok=True)
        with open(a.csv, "w") as f:
            f.write("restored,grad_restored" + (",gt,edge,gmsd,grad_gt,grad_ratio" if a.gt else "") + "\n")
            for it, m in zip(a.items, res):
                tail = f",{it[1]},{m['edge']!r},{m['gmsd']!r},{m['grad_gt']!r},{m['grad_ratio']!r}" if a.gt else ""
                f.write(f"{it[0]},{m['grad_restored']!r}{tail}\n")


if __name__ == "__main__":
    main()
