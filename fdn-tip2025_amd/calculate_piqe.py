"""PIQE of a folder of images on the HIP path: the no-reference score the unpaired low-light sets (DICM, LIME, MEF, NPE, VV,
Real-LOL-Blur) are reported with beside NIQE and LOE, for output sets that have no ground truth.  Unlike NIQE it needs no parameter
file: include/fdn_piqe.h is the whole definition (written out from Venkatanath et al., NCC 2015, and MATLAB's documented constants; no
comparison against MATLAB or pyiqa has been made).  0 is best, 100 is worst; an image without one active 16 x 16 block (a flat image)
scores exactly 100.  Frames of equal size are scored as one batch.  Needs a ROCm GPU and the built libfdn_piqe.so; there is no CPU
fallback.

    python calculate_piqe.py --input 'results/realblur_FDN/*.png'
    python calculate_piqe.py --input results/DICM --csv piqe.csv --masks results/DICM_masks

Images are decoded with PIL: 8-bit greyscale ('L') or RGB.  16-bit images are refused; an alpha channel is refused unless --drop_alpha
is given.  --csv writes one line `image,piqe,active_blocks` per image.  --masks DIR writes, per image, <name>_active.png, <name>_wndc.png
and <name>_wnc.png: MATLAB's three masks (the active blocks, those with a noticeable distortion, those with noise), every 16 x 16 block
one value, 0 or 255, upscaled to the image's size.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from calculate_niqe import list_images  # noqa: E402

MASKS = (("active", 1), ("wndc", 2), ("wnc", 4))                          # file suffix, bit of the class byte (include/fdn_piqe.h)


def load_rgb(path, drop_alpha=False):
    """-> uint8 (h, w, 3) in R, G, B order; a greyscale image has its plane in all three (its gray code is the plane)"""
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
    return np.ascontiguousarray(np.repeat(a[..., None], 3, axis=2) if a.ndim == 2 else a)


def mask_images(cls, h, w):
    """class bytes [H/16][W/16] of an h x w image -> {suffix: uint8 (h, w) of 0 / 255}, every block upscaled to its 16 x 16 pixels"""
    out = {}
    for name, bit in MASKS:
        m = ((np.asarray(cls) & bit) != 0).astype(np.uint8) * 255
        out[name] = np.ascontiguousarray(np.repeat(np.repeat(m, 16, axis=0), 16, axis=1)[:h, :w])
    return out


def image_size(path):
    """-> (h, w) from the file's header: nothing is decoded"""
    from PIL import Image
    with Image.open(path) as im:
        return im.size[1], im.size[0]


def score_all(paths, batch=8, device="cuda:0", drop_alpha=False, masks=None):
    """-> one record {piqe, d, nhsa} per path, in order; images of equal size go to the GPU together, up to `batch` at a time.  The
    sizes come from the files' headers and only one batch is decoded at a time, so a folder of any length is scored in the memory of
    `batch` images.  masks: a folder for the three block masks of every image."""
    import torch
    from fdn_hip import piqe
    groups = {}
    for i, p in enumerate(paths):
        groups.setdefault(image_size(p), []).append(i)
    recs = [None] * len(paths)
    dev = torch.device(device)
    if masks:
        os.makedirs(masks, exist_ok=True)
    with torch.cuda.device(dev):
        for (h, w), idx in groups.items():
            for k in range(0, len(idx), max(1, batch)):
                chunk = idx[k:k + max(1, batch)]
                x = torch.from_numpy(np.stack([load_rgb(paths[i], drop_alpha) for i in chunk])).to(dev)
                if masks:
                    r, m = piqe.piqe_u8(x, bgr=False, maps=True)
                    cls = m["cls"].cpu().numpy()
                    from PIL import Image
                    for j, i in enumerate(chunk):
                        stem = os.path.splitext(os.path.basename(paths[i]))[0]
                        for name, im in mask_images(cls[j], h, w).items():
                            Image.fromarray(im).save(os.path.join(masks, f"{stem}_{name}.png"))
                else:
                    r = piqe.piqe_u8(x, bgr=False)
                for i, s in zip(chunk, r):
                    recs[i] = s
    return recs


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--input", required=True, help="images: a glob ('out/*.png', 'out/**/*.png') or a folder")
    ap.add_argument("--batch", type=int, default=8, help="images of equal size scored per launch")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--drop_alpha", action="store_true", help="score RGBA / LA images without their alpha channel")
    ap.add_argument("--csv", default=None, metavar="PATH", help="write image,piqe,active_blocks per image there, floats as repr() writes them")
    ap.add_argument("--masks", default=None, metavar="DIR", help="write the three block masks of every image there as PNGs of the image's size")
    a = ap.parse_args(argv)
    if a.batch < 1:
        ap.error("--batch must be at least 1")
    a.paths = list_images(a.input)
    if not a.paths:
        ap.error(f"no images match {a.input!r}")
    return a


def main(argv=None):
    a = parse_args(argv)
    try:
        recs = score_all(a.paths, a.batch, a.device, a.drop_alpha, a.masks)
    except ValueError as e:
        sys.exit(f"calculate_piqe.py: {e}")
    from fdn_hip.piqe import piqe_line
    for i, (p, r) in enumerate(zip(a.paths, recs)):
        basename, _ = os.path.splitext(os.path.basename(p))
        print(f'{i+1:3d}: {basename:25}. \t{piqe_line(r)}')
    print(a.input)
    print(f'Average: PIQE: {sum(r["piqe"] for r in recs) / len(recs):.6f}')
    if a.csv:
        os.makedirs(os.path.dirname(a.csv) or ".", exist_ok=True)
        with open(a.csv, "w") as f:
            f.write("image,piqe,active_blocks\n")
            for p, r in zip(a.paths, recs):
                f.write(f"{p},{r['piqe']!r},{r['nhsa']}\n")


if __name__ == "__main__":
    main()
