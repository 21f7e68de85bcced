"""Ratio sweep on the HIP path: the role of the reference's inference_fdn_multi_r.py:52-85 - ONE low-light frame enhanced with the
illumination ratio forced to every value of a grid (the reference: `for i in np.arange(0, 1, 0.01)`, `ratio = ratio / ratio * i`,
results written to ./multi_r/<i>.png), here with the grid values of the sweep as the BATCH of one forward per chunk: the frame is
repeated, ratio_i carries the grid, LPNet is not needed (its prediction only supplied the shape in the reference).

    python inference_fdn_multi_r.py --fdn FDN_lolblur.pth --input frame.png --output multi_r/ [--start 0 --stop 1 --step 0.01]

--tile HxW|auto runs a frame larger than one forward can take as overlapping tiles (fdn_hip.harness.enhance_u8), one grid value at a time;
--tile-blend feather merges them with ramps across their overlaps instead of the uniform average.  --ensemble 2|4|8 averages FDN's results
on that many flipped / transposed copies of the frame (fdn_hip.ensemble), each fed the grid value.  --fuse also writes fused.png, the
exposure fusion (fdn_hip.fusion) of the frame's renderings at the grid's values, at most 16 of them (choose --start / --stop / --step
accordingly); --fusion-weights C,S,E are the exponents of contrast, saturation and well-exposedness in its weights.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from inference_fdn_lolblur import (add_ensemble_arg, add_tile_args, fusion_weights_arg, hint_hard_seam, hint_large_frame, load_params,  # noqa: E402
                                   read_rgb, write_rgb)


def sweep_values(start, stop, step):
    """np.arange(start, stop, step) as the reference walks it (inference_fdn_multi_r.py:55)."""
    return np.arange(start, stop, step)


def output_name(v):
    """The reference formats the loop variable itself: './multi_r/{}.png'.format(i) (:84)."""
    return "{}.png".format(v)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--fdn", required=True, help="FDN checkpoint ({'params': state_dict}, 1503 keys)")
    ap.add_argument("--input", required=True, help="one input frame")
    ap.add_argument("--output", default="multi_r", help="output directory (the reference: ./multi_r)")
    ap.add_argument("--start", type=float, default=0.0)
    ap.add_argument("--stop", type=float, default=1.0)
    ap.add_argument("--step", type=float, default=0.01)
    ap.add_argument("--batch", type=int, default=8, help="grid values per forward")
    ap.add_argument("--device", default="cuda:0")
    add_tile_args(ap, ratio_default=None)                     # the sweep's ratio is fixed: nothing to take from a frame or a tile
    add_ensemble_arg(ap)
    ap.add_argument("--fuse", action="store_true", help="also write fused.png: the exposure fusion of the renderings at the grid's values")
    ap.add_argument("--fusion-weights", type=fusion_weights_arg, default=(1.0, 1.0, 1.0), metavar="C,S,E",
                    help="with --fuse: the exponents of contrast, saturation and well-exposedness in the fusion's weights (default 1,1,1)")
    a = ap.parse_args(argv)
    if a.fuse:
        n = len(sweep_values(a.start, a.stop, a.step))
        if not 1 <= n <= 16:
            ap.error(f"--fuse takes a grid of 1 to 16 values, this one has {n}: choose a wider --step (or another --start / --stop)")
    return a


def main(argv=None):
    a = parse_args(argv)

    from basicsr.models.archs.FDN_arch import FDN
    from fdn_hip.harness import enhance_u8

    dev = torch.device(a.device)
    torch.cuda.set_device(dev)
    net = FDN().to(dev).eval()
    net.load_state_dict(load_params(a.fdn), strict=True)
    img = torch.from_numpy(read_rgb(a.input)).to(dev)
    hint_large_frame(a.tile, img.shape[0], img.shape[1])
    hint_hard_seam(a.tile, a.tile_blend, a.tile_overlap, img.shape[0], img.shape[1])
    vals = sweep_values(a.start, a.stop, a.step)
    for c0 in range(0, len(vals), a.batch):
        chunk = vals[c0:c0 + a.batch]
        ratio = torch.tensor(chunk, dtype=torch.float32, device=dev).view(-1, 1)
        out = enhance_u8(net, None, img.unsqueeze(0).expand(len(chunk), -1, -1, -1).contiguous(), bgr=False, ratio_mode="fixed", ratio=ratio,
                         tile=a.tile, overlap=a.tile_overlap, batch=a.batch, blend=a.tile_blend, ensemble=a.ensemble)
        for v, o in zip(chunk, out.cpu().numpy()):
            write_rgb(os.path.join(a.output, output_name(v)), o)
    if a.fuse:
        from fdn_hip import fusion
        from fdn_hip.harness import postprocess, render_ratios, resolve_tile
        frames, h, w = render_ratios(net, img, torch.tensor(vals, dtype=torch.float32, device=dev).view(-1, 1), bgr=False,
                                     tile=resolve_tile(a.tile, img.shape[0], img.shape[1]), overlap=a.tile_overlap, batch=a.batch,
                                     blend=a.tile_blend, ensemble=a.ensemble)
        fused = postprocess(fusion.fuse(frames, h, w, a.fusion_weights).unsqueeze(0), h, w, bgr=False)[0]
        write_rgb(os.path.join(a.output, "fused.png"), fused.cpu().numpy())
    print(f"{len(vals)} ratios -> {a.output}")


if __name__ == "__main__":
    main()
