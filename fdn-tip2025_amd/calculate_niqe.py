"""NIQE of a folder of images on the HIP path: the role of the reference's scripts/metrics/calculate_niqe.py (calculate_niqe with
crop_border, input_order='HWC', convert_to='y' per image, then the average), for output sets that have no ground truth.  Frames of
equal size are scored as one batch.  Needs a ROCm GPU and the built libfdn_hip.so; there is no CPU fallback.

    python calculate_niqe.py --input 'results/realblur_FDN/*.png' --params /path/to/FDN-TIP2025/basicsr/metrics/niqe_pris_params.npz

Images are decoded with PIL: 8-bit greyscale ('L', scored as the reference scores a 1-channel image) or RGB (put in B, G, R order, as
cv2.imread gives).  16-bit images are refused; an alpha channel is refused unless --drop_alpha is given.
"""
import argparse
import glob
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

IMG_EXT = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff", ".ppm", ".pgm", ".webp")


def list_images(pattern):
    """a glob (recursive '**' allowed), or a folder: every image under it, as the reference's scandir(recursive=True); sorted"""
    if os.path.isdir(pattern):
        pattern = os.path.join(pattern, "**", "*")
    return sorted(p for p in glob.glob(pattern, recursive=True) if os.path.isfile(p) and p.lower().endswith(IMG_EXT))


def load_bgr(path, drop_alpha=False):
    """-> float32 (C, H, W) in [0, 255]: C = 3 in B, G, R order, or C = 1 for greyscale"""
    from PIL import Image
    with Image.open(path) as im:
        mode = im.mode
        if any(";16" in str(t[3]) for t in (im.tile or [])):                  # PIL opens a 48-bit PNG as 'RGB', dropping 8 bits
            raise ValueError(f"{path}: 16-bit images are not scored (only 8-bit greyscale or RGB)")
        if mode in ("RGBA", "LA") and drop_alpha:
            im = im.convert("RGB" if mode == "RGBA" else "L")
            mode = im.mode
        if mode in ("RGBA", "LA", "PA"):
            raise ValueError(f"{path}: image has an alpha channel (mode {mode}); pass --drop_alpha to score it without")
        if mode not in ("L", "RGB"):
            raise ValueError(f"{path}: only 8-bit greyscale or RGB images are scored (mode {mode})")
        a = np.array(im, dtype=np.uint8)
    if a.ndim == 2:
        return a[None].astype(np.float32)
    return np.ascontiguousarray(a[..., ::-1].transpose(2, 0, 1)).astype(np.float32)


def score_all(paths, crop_border=0, params=None, batch=8, device="cuda:0", drop_alpha=False):
    """-> NIQE per path, in order; images of equal shape go to the GPU together, up to `batch` at a time"""
    import torch
    from fdn_hip import metrics
    params = metrics.niqe_params(params)
    pris = {"mu_pris_param": params[0], "cov_pris_param": params[1], "gaussian_window": params[2]}
    imgs = [load_bgr(p, drop_alpha) for p in paths]
    groups = {}
    for i, a in enumerate(imgs):
        groups.setdefault(a.shape, []).append(i)
    scores = [None] * len(paths)
    dev = torch.device(device)
    with torch.cuda.device(dev):
        for idx in groups.values():
            for k in range(0, len(idx), max(1, batch)):
                chunk = idx[k:k + max(1, batch)]
                x = torch.from_numpy(np.stack([imgs[i] for i in chunk])).to(dev)
                q = metrics.calculate_niqe(x, crop_border, input_order="CHW", convert_to="y", params=pris)
                for i, s in zip(chunk, q if isinstance(q, list) else [q]):
                    scores[i] = s
    return scores


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--input", required=True, help="images: a glob ('out/*.png', 'out/**/*.png') or a folder")
    ap.add_argument("--crop_border", type=int, default=0, help="Crop border for each side")
    ap.add_argument("--params", default=None, help="niqe_pris_params.npz (default: basicsr/metrics/ of the reference checkout on sys.path)")
    ap.add_argument("--batch", type=int, default=8, help="images of equal size scored per launch")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--drop_alpha", action="store_true", help="score RGBA / LA images without their alpha channel")
    args = ap.parse_args(argv)
    paths = list_images(args.input)
    if not paths:
        ap.error(f"no images match {args.input!r}")
    scores = score_all(paths, args.crop_border, args.params, args.batch, args.device, args.drop_alpha)
    for i, (p, s) in enumerate(zip(paths, scores)):
        basename, _ = os.path.splitext(os.path.basename(p))
        print(f'{i+1:3d}: {basename:25}. \tNIQE: {s:.6f}')
    print(args.input)
    print(f'Average: NIQE: {sum(scores) / len(scores):.6f}')


if __name__ == "__main__":
    main()
