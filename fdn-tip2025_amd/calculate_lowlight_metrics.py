"""The two scores a low-light enhancer is judged by, on the HIP path (fdn_hip.lowlight): the lightness order error LOE of every input
image against its enhanced version (after Wang et al. 2013; no ground truth needed, so it is the score for real footage), and with --gt
the CIEDE2000 colour difference dE00 of the enhanced image against its ground truth (mean and maximum over the pixels).  The globs are
sorted and paired by index; unequal counts and unequal sizes within a pair are errors.  Pairs of equal size are scored as one batch, with
one device-to-host copy per batch.  Needs a ROCm GPU and the built libfdn_hip.so; there is no CPU fallback.  Images must be 8-bit RGB.

    python calculate_lowlight_metrics.py --input 'lolblur/test/low_blur/*/*' --restored 'results/lolblur/*/*' \\
        --gt 'lolblur/test/high_sharp_scaled/*/*' --csv lowlight.csv

--loe-size N samples a grid whose short side has N points (50, the usual choice: scores comparable in scale to published ones, though
the sampling rule is this project's own); 0 scores every pixel, which costs hardly more here.  --save-loe-map DIR writes, per image, the
share of the samples whose lightness order against each sample was reversed (RD / m) as an 8-bit grey PNG of the sample grid.
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


def match_paths(input_glob, restored_glob, gt_glob=None):
    """the sorted globs paired by index -> [(input, restored)] or [(input, restored, gt)]"""
    inp, rs = sorted(glob.glob(input_glob)), sorted(glob.glob(restored_glob))
    if not inp:
        raise ValueError(f"no input images match {input_glob!r}")
    if len(inp) != len(rs):
        raise ValueError(f"{len(inp)} input images ({input_glob!r}) but {len(rs)} restored ({restored_glob!r})")
    if gt_glob is None:
        return list(zip(inp, rs))
    return [(i, r, g) for i, (g, r) in zip(inp, pair_paths(gt_glob, restored_glob))]


def decoded_groups(items, batch, pool):
    """tuples of 2 or 3 paths -> (indices, [images [n][h][w][3] per position]) per group of tuples of one size, at most `batch` each;
    the group handed out and the next one, decoding on `pool` meanwhile, are all that is in host memory"""
    shapes = [[image_shape(p) for p in it] for it in items]
    for i, s in enumerate(shapes):
        if len(s) == 3 and tuple(s[2]) != tuple(s[1]):
            raise ValueError(f"pair {i + 1}: ground truth {tuple(s[2])} and restored {tuple(s[1])} differ in size")
    try:
        groups = group_pairs([(s[0], s[1]) for s in shapes], batch)
    except ValueError as e:
        raise ValueError(str(e).replace("ground truth", "input")) from None
    width = len(items[0])

    def submit(idx):
        return [[pool.submit(read_rgb8, items[i][k]) for i in idx] for k in range(width)]
    ahead = submit(groups[0])
    for n, idx in enumerate(groups):
        now, ahead = ahead, submit(groups[n + 1]) if n + 1 < len(groups) else None
        yield idx, [np.stack([f.result() for f in col]) for col in now]


def score(items, size=50, batch=8, device="cuda:0", save_map=None, workers=4):
    """-> one dict of fdn_hip.lowlight.lowlight_metrics per tuple of paths, in order"""
    import torch
    from fdn_hip import lowlight
    dev = torch.device(device)
    torch.cuda.set_device(dev)
    out = [None] * len(items)
    with ThreadPoolExecutor(max_workers=workers) as pool:
        for idx, cols in decoded_groups(items, batch, pool):
            t = [torch.from_numpy(c).to(dev) for c in cols]
            res = lowlight.lowlight_metrics(t[0], t[1], t[2] if len(t) == 3 else None, size=size, bgr=False, want_loe_map=bool(save_map))
            if save_map:
                res, maps = res[0], res[1].cpu().numpy()
            for k, i in enumerate(idx):
                out[i] = res[k]
                if save_map:
                    write_map(os.path.join(save_map, os.path.splitext(os.path.basename(items[i][1]))[0] + ".png"), maps[k],
                              res[k]["loe_samples"])
    return out


def map_bytes(rd, m):
    """RD of every sample and the number of samples -> the 8-bit picture of RD / m"""
    return np.rint(rd.astype(np.float64) * (255.0 / m)).astype(np.uint8)


def write_map(path, rd, m):
    from PIL import Image
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    Image.fromarray(map_bytes(rd, m), mode="L").save(path)


def lowlight_line(m):
    """the figures of one image, as printed here and by validate_fdn.py --lowlight"""
    line = f"LOE: {m['loe']:.6f}"
    if "deltae" in m:
        line += f", dE00: {m['deltae']:.6f}"
    return line


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--input", required=True, help="the low-light input images: a glob, sorted")
    ap.add_argument("--restored", required=True, help="the enhanced images: a glob, sorted and paired with --input by index")
    ap.add_argument("--gt", default=None, help="ground-truth images for dE00: a glob, sorted and paired by index; without it LOE only")
    ap.add_argument("--loe-size", type=int, default=50, help="points along the short side of LOE's sample grid; 0 = full resolution")
    ap.add_argument("--batch", type=int, default=8, help="images of equal size scored per launch")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--csv", default=None, help="file for one line per image")
    ap.add_argument("--save-loe-map", default=None, metavar="DIR", help="directory for the RD / m pictures, one 8-bit grey PNG per image")
    a = ap.parse_args(argv)
    if a.loe_size < 0:
        ap.error("--loe-size must be >= 0")
    if a.batch < 1:
        ap.error("--batch must be >= 1")
    try:
        a.items = match_paths(a.input, a.restored, a.gt)
    except ValueError as e:
        ap.error(str(e))
    return a


def main(argv=None):
    a = parse_args(argv)
    from fdn_hip import FdnHipError
    try:
        res = score(a.items, a.loe_size, a.batch, a.device, a.save_loe_map)
    except (FdnHipError, ValueError) as e:
        sys.exit(f"calculate_lowlight_metrics.py: {e}")
    for i, (it, m) in enumerate(zip(a.items, res)):
        basename = os.path.splitext(os.path.basename(it[1]))[0]
        tail = f" (max {m['deltae_max']:.6f})" if a.gt else ""
        print(f"{i+1:3d}: {basename:25}. \t{lowlight_line(m)}{tail}")
    avg = {k: sum(m[k] for m in res) / len(res) for k in (("loe", "deltae") if a.gt else ("loe",))}
    print(f"Average: {lowlight_line(avg)}")
    if a.csv:
        os.makedirs(os.path.dirname(a.csv) or ".", exist_ok=True)
        with open(a.csv, "w") as f:
            f.write("input,restored,loe,loe_numerator,loe_samples" + (",gt,deltae,deltae_max" if a.gt else "") + "\n")
            for it, m in zip(a.items, res):
                tail = f",{it[2]},{m['deltae']!r},{m['deltae_max']!r}" if a.gt else ""
                f.write(f"{it[0]},{it[1]},{m['loe']!r},{m['loe_numerator']},{m['loe_samples']}{tail}\n")


if __name__ == "__main__":
    main()
