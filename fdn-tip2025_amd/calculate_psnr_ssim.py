"""PSNR and SSIM of restored images against their ground truth on the HIP path: the role of the reference's
scripts/metrics/calculate_psnr_ssim.py (calculate_psnr / calculate_ssim of basicsr/metrics/psnr_ssim.py, RGB channels, the 3-D SSIM).
Both globs are sorted and paired by index; unequal counts are an error here.  Pairs of equal size are scored as one batch, with one
device-to-host copy per batch.  Needs a ROCm GPU and the built libfdn_hip.so; there is no CPU fallback.

    python calculate_psnr_ssim.py --gt 'lolblur/test/high_sharp_scaled/*/*' --restored 'results/lolblur/*/*'

The reference scores float32(byte) / 255. * 255. (:31, :36, :61), which in float32 is the byte again for all 256 values, so the bytes
are scored as they are; the ground truth is img1, whose maximum picks the peak value, as there.  --test_y_channel scores the Y channel
of BT.601 (calculate_psnr / calculate_ssim with test_y_channel=True), image by image.  The reference's --correct_mean_var (an
affine correction of the restored image before scoring) is not offered.  Images are decoded with PIL on worker threads and must be 8-bit RGB.
"""
import argparse
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from calculate_lpips import group_pairs, pair_paths, read_rgb8  # noqa: E402


def image_shape(path):
    """(h, w, 3) from the file's header, without decoding it"""
    from PIL import Image
    with Image.open(path) as im:
        return (im.height, im.width, 3)


def decoded_groups(pairs, batch, pool):
    """pairs of paths -> (pair indices, first images [n][h][w][3], second images) per group of pairs of one size, at most `batch` each.
    The sizes come from the headers; only the group handed out and the next one, decoding on `pool` meanwhile, are in host memory, so
    a whole test set never is."""
    groups = group_pairs([(image_shape(a), image_shape(b)) for a, b in pairs], batch)

    def submit(idx):
        return [[pool.submit(read_rgb8, pairs[i][k]) for i in idx] for k in (0, 1)]
    ahead = submit(groups[0])
    for n, idx in enumerate(groups):
        now, ahead = ahead, submit(groups[n + 1]) if n + 1 < len(groups) else None
        yield idx, np.stack([f.result() for f in now[0]]), np.stack([f.result() for f in now[1]])


def score_pairs(pairs, crop_border=0, test_y_channel=False, batch=8, device="cuda:0", workers=4):
    """-> (PSNR, SSIM) per (gt, restored) pair, in order; the ground truth is img1, as in the reference script (:61-62)"""
    import torch
    from fdn_hip import metrics
    dev = torch.device(device)
    psnr, ssim = [None] * len(pairs), [None] * len(pairs)
    with ThreadPoolExecutor(max_workers=workers) as pool:
        for idx, gts, rss in decoded_groups(pairs, batch, pool):
            a, b = torch.from_numpy(gts).to(dev), torch.from_numpy(rss).to(dev)
            p, s = metrics.calculate_psnr_ssim_u8(a, b, crop_border=crop_border, test_y_channel=test_y_channel, bgr=False)
            for k, i in enumerate(idx):
                psnr[i], ssim[i] = p[k], s[k]
    return psnr, ssim


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gt", required=True, help="ground-truth images: a glob, sorted")
    ap.add_argument("--restored", required=True, help="restored images: a glob, sorted and paired with --gt by index")
    ap.add_argument("--crop_border", type=int, default=0, help="pixels cut from every edge before scoring")
    ap.add_argument("--test_y_channel", action="store_true", help="score the Y channel (MATLAB YCbCr) instead of the RGB channels")
    ap.add_argument("--batch", type=int, default=8, help="pairs of equal size scored per launch")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if args.crop_border < 0:
        ap.error("--crop_border must be >= 0")
    try:
        pairs = pair_paths(args.gt, args.restored)
    except ValueError as e:
        ap.error(str(e))
    print('Testing Y channel.' if args.test_y_channel else 'Testing RGB channels.')
    psnr_all, ssim_all = score_pairs(pairs, args.crop_border, args.test_y_channel, args.batch, args.device)
    for i, ((gt, _), psnr, ssim) in enumerate(zip(pairs, psnr_all, ssim_all)):
        basename = os.path.splitext(os.path.basename(gt))[0]
        print(f'{i+1:3d}: {basename:25}. \tPSNR: {psnr:.6f} dB, \tSSIM: {ssim:.6f}')
    print(f'Average: PSNR: {sum(psnr_all) / len(psnr_all):.6f} dB, SSIM: {sum(ssim_all) / len(ssim_all):.6f}')


if __name__ == "__main__":
    main()
