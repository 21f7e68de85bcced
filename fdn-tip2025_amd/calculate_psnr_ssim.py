"""PSNR and SSIM of restored images against their ground truth on the HIP path: the role of the reference's
scripts/metrics/calculate_psnr_ssim.py (calculate_psnr / calculate_ssim of basicsr/metrics/psnr_ssim.py, RGB channels, the 3-D SSIM).
Both globs are sorted and paired by index; unequal counts are an error here.  Pairs of equal size are scored as one batch, with one
device-to-host copy per batch.  Needs a ROCm GPU and the built libfdn_hip.so; there is no CPU fallback.

    python calculate_psnr_ssim.py --gt 'lolblur/test/high_sharp_scaled/*/*' --restored 'results/lolblur/*/*'

The reference scores float32(byte) / 255. * 255. (:31, :36, :61), which in float32 is the byte again for all 256 values, so the bytes
are scored as they are; the ground truth is img1, whose maximum picks the peak value, as there.  --test_y_channel scores the Y channel
of BT.601 (calculate_psnr / calculate_ssim with test_y_channel=True), image by image.  --correct mean_var scores the restored image
after every channel has been shifted and scaled to the ground truth's mean and standard deviation, what the reference's
--correct_mean_var does (:38-54; the flag itself is not offered, it is spelt --correct mean_var here); --correct gt_mean after the
restored image has been multiplied by mean(gray(gt)) / mean(gray(restored)) and clipped, the GT-mean convention of KinD, LLFlow and
Retinexformer, which the reference does not have (fdn_hip/correct.py defines both).  An image without a correction (a flat restored
channel, a black restored image) scores nan; it is named on stderr and the exit status is 1.  Images are decoded with PIL on worker
threads and must be 8-bit RGB.
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


def score_pairs(pairs, crop_border=0, test_y_channel=False, batch=8, device="cuda:0", workers=4, correct=None):
    """-> (PSNR, SSIM) per (gt, restored) pair, in order; the ground truth is img1, as in the reference script (:61-62).
    correct: None, or "gt_mean" / "mean_var": the scores of the corrected restored image (fdn_hip.correct)"""
    import torch
    from fdn_hip import metrics
    if correct:
        from fdn_hip.correct import calculate_psnr_ssim_corrected_u8
    dev = torch.device(device)
    psnr, ssim = [None] * len(pairs), [None] * len(pairs)
    with ThreadPoolExecutor(max_workers=workers) as pool:
        for idx, gts, rss in decoded_groups(pairs, batch, pool):
            a, b = torch.from_numpy(gts).to(dev), torch.from_numpy(rss).to(dev)
            if correct:
                p, s = calculate_psnr_ssim_corrected_u8(a, b, correct, crop_border=crop_border, test_y_channel=test_y_channel, bgr=False)
            else:
                p, s = metrics.calculate_psnr_ssim_u8(a, b, crop_border=crop_border, test_y_channel=test_y_channel, bgr=False)
            for k, i in enumerate(idx):
                psnr[i], ssim[i] = p[k], s[k]
    return psnr, ssim


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gt", required=True, help="ground-truth images: a glob, sorted")
    ap.add_argument("--restored", required=True, help="restored images: a glob, sorted and paired with --gt by index")
    ap.add_argument("--crop_border", type=int, default=0, help="pixels cut from every edge before scoring")
    ap.add_argument("--test_y_channel", action="store_true", help="score the Y channel (MATLAB YCbCr) instead of the RGB channels")
    ap.add_argument("--batch", type=int, default=8, help="pairs of equal size scored per launch")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--correct", choices=("gt_mean", "mean_var"), default=None,
                    help="score the restored image after a brightness correction towards the ground truth: mean_var, every channel to the "
                         "ground truth's mean and standard deviation; gt_mean, the image times the ratio of the mean grays, clipped")
    ap.add_argument("--correct_mean_var", action="store_true", help="not offered under this name: use --correct mean_var")
    args = ap.parse_args(argv)
    if args.correct_mean_var:
        ap.error("--correct_mean_var is not offered under this name: use --correct mean_var")
    if args.crop_border < 0:
        ap.error("--crop_border must be >= 0")
    try:
        args.pairs = pair_paths(args.gt, args.restored)
    except ValueError as e:
        ap.error(str(e))
    return args


def main(argv=None):
    args = parse_args(argv)
    pairs = args.pairs
    print(('Testing Y channel.' if args.test_y_channel else 'Testing RGB channels.') + (f' Correction: {args.correct}.' if args.correct else ''))
    psnr_all, ssim_all = score_pairs(pairs, args.crop_border, args.test_y_channel, args.batch, args.device, correct=args.correct)
    bad = []
    for i, ((gt, restored), psnr, ssim) in enumerate(zip(pairs, psnr_all, ssim_all)):
        basename = os.path.splitext(os.path.basename(gt))[0]
        print(f'{i+1:3d}: {basename:25}. \tPSNR: {psnr:.6f} dB, \tSSIM: {ssim:.6f}')
        if psnr != psnr or ssim != ssim:
            bad.append(restored)
    print(f'Average: PSNR: {sum(psnr_all) / len(psnr_all):.6f} dB, SSIM: {sum(ssim_all) / len(ssim_all):.6f}')
    for path in bad:
        print(f"calculate_psnr_ssim.py: --correct {args.correct}: {path} has no correction (a flat channel or a black image): nan", file=sys.stderr)
    if bad:
        sys.exit(1)


if __name__ == "__main__":
    main()
