"""LPIPS of restored images against their ground truth on the HIP path: the role of the reference's scripts/metrics/calculate_lpips.py
(lpips.LPIPS(net='vgg'), version 0.1).  Both globs are sorted and paired by index, as the reference pairs them; unequal counts are an
error here.  Pairs of equal size are scored as one batch.  Needs a ROCm GPU and the built libfdn_hip.so; there is no CPU fallback.

    python calculate_lpips.py --gt 'lolblur/test/high_sharp_scaled/*/*' --restored 'results/lolblur/*/*' \\
        --net vgg --weights vgg16-397923af.pth --lin lpips/weights/v0.1/vgg.pth

--weights is an lpips.LPIPS state_dict (then --lin only if it lacks the linear heads), or a torchvision vgg16 / alexnet state_dict with
--lin, the lpips package's weights/v0.1/{vgg,alex}.pth.  Images are decoded with PIL on worker threads and must be
8-bit RGB.
"""
import argparse
import glob
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def pair_paths(gt_glob, restored_glob):
    """sorted(glob(gt)) and sorted(glob(restored)), paired by index"""
    gt, rs = sorted(glob.glob(gt_glob)), sorted(glob.glob(restored_glob))
    if not gt:
        raise ValueError(f"no ground-truth images match {gt_glob!r}")
    if len(gt) != len(rs):
        raise ValueError(f"{len(gt)} ground-truth images ({gt_glob!r}) but {len(rs)} restored ({restored_glob!r})")
    return list(zip(gt, rs))


def read_rgb8(path):
    """-> uint8 (H, W, 3), R, G, B; anything but an 8-bit RGB image is refused"""
    from PIL import Image
    with Image.open(path) as im:
        if any(";16" in str(t[3]) for t in (im.tile or [])) or im.mode != "RGB":      # PIL opens a 48-bit PNG as 'RGB'
            raise ValueError(f"{path}: only 8-bit RGB images are scored (mode {im.mode}{', 16-bit' if im.mode == 'RGB' else ''})")
        return np.array(im, dtype=np.uint8)


def group_pairs(shapes, batch):
    """shapes[i] = (gt shape, restored shape) of pair i -> [[pair indices]]: pairs of one size, at most `batch` per group, in order of
    first appearance; a pair whose two images differ in size is an error"""
    groups = {}
    for i, (a, b) in enumerate(shapes):
        if tuple(a) != tuple(b):
            raise ValueError(f"pair {i + 1}: ground truth {tuple(a)} and restored {tuple(b)} differ in size")
        groups.setdefault(tuple(a), []).append(i)
    n = max(1, batch)
    return [idx[k:k + n] for idx in groups.values() for k in range(0, len(idx), n)]


def score_pairs(pairs, net="vgg", weights=None, lin_weights=None, batch=8, device="cuda:0", workers=4):
    """-> LPIPS per (gt, restored) pair, in order; the restored image is lpips' in0, as in the reference"""
    import torch
    from fdn_hip import metrics
    with ThreadPoolExecutor(max_workers=workers) as pool:
        gts = list(pool.map(read_rgb8, [g for g, _ in pairs]))
        rss = list(pool.map(read_rgb8, [r for _, r in pairs]))
    dev = torch.device(device)
    model = metrics.lpips_model(net, weights, lin_weights, dev)
    scores = [None] * len(pairs)
    for idx in group_pairs([(g.shape, r.shape) for g, r in zip(gts, rss)], batch):
        a = np.stack([rss[i] for i in idx])
        b = np.stack([gts[i] for i in idx])
        d = metrics.calculate_lpips(a, b, model=model, bgr=False)
        for i, s in zip(idx, d if isinstance(d, list) else [d]):
            scores[i] = s
    return scores


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gt", required=True, help="ground-truth images: a glob, sorted")
    ap.add_argument("--restored", required=True, help="restored images: a glob, sorted and paired with --gt by index")
    ap.add_argument("--net", choices=("vgg", "alex"), default="vgg")
    ap.add_argument("--weights", required=True, help="lpips.LPIPS state_dict, or torchvision backbone state_dict (with --lin)")
    ap.add_argument("--lin", default=None, help="the lpips linear heads, weights/v0.1/{vgg,alex}.pth")
    ap.add_argument("--batch", type=int, default=8, help="pairs of equal size scored per backbone pass")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    try:
        pairs = pair_paths(args.gt, args.restored)
    except ValueError as e:
        ap.error(str(e))
    scores = score_pairs(pairs, args.net, args.weights, args.lin, args.batch, args.device)
    for i, s in enumerate(scores):
        print(f'{i+1:3d}: . \tLPIPS: {s:.6f}.')
    print(f'Average: LPIPS: {sum(scores) / len(scores):.6f}')


if __name__ == "__main__":
    main()
