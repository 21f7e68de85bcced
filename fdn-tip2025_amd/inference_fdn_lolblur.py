"""LOL-Blur inference driver on the HIP path: the role of the reference's inference_fdn_lolblur.py:1-75
(load LPNet + FDN checkpoints, walk a directory of low-light blurry frames, write the enhanced frames), with
the paths as arguments instead of constants and the per-image host work moved to the GPU:

    decode (PIL, worker threads)  ->  uint8 HWC on the GPU  ->  fdn_pre_u8  ->  LPNet -> FDN  ->  fdn_post_u8  ->  encode

Images of equal size are batched (the reference runs batch 1; every op of the path is per-sample).
Needs a ROCm GPU and the built libfdn_hip.so; there is no CPU fallback.

    python inference_fdn_lolblur.py --fdn FDN_lolblur.pth --lpnet LPNet_lolblur.pth --input 'frames/*.png' --output out/

A frame larger than one forward can take (a 12 MP photo) runs with --tile HxW or --tile auto: overlapping tiles as the reference's
val.grids cuts them, each through FDN, averaged where they overlap (--tile-blend feather: weighted with ramps across the overlaps, so that
no step runs along the line where a tile ends; --tile-overlap sets the least width of those bands); the ratio comes from the whole frame
(--tile-ratio frame) or from each tile (tile: the reference's semantics).  Under `python -m torch.distributed.run --nproc_per_node N`
with --tile, rank 0 reads, splits, merges and writes, and the tiles of each frame are dealt to all N GPUs.

--ensemble 2|4|8 is the geometric self-ensemble (fdn_hip.ensemble): every frame - or every tile - runs through FDN in that many flipped /
transposed copies with the ratio of the untransformed frame, and the results, mapped back, are averaged: 2, 4 or 8 forwards per frame.
One GPU only.  No accuracy gain has been measured with it here (no trained checkpoint at hand).

--ratio VALUE feeds FDN that ratio for every frame instead of LPNet's (--lpnet is then not needed).  --bracket EV[,EV...] (for example
-1,0,1) renders every frame at the ratio it would be fed times 2^-EV for every stop (a positive stop is brighter) and fuses the renderings
into one locally exposed frame (fdn_hip.fusion: exposure fusion, Mertens et al. 2007): one forward per stop and frame.  --fusion-weights
C,S,E are the exponents of contrast, saturation and well-exposedness in the fusion's weights (default 1,1,1).  No gain in any quality
figure has been measured with it here (no trained checkpoint at hand).
"""
import argparse
import glob
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def read_rgb(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert("RGB"), dtype=np.uint8)           # (a copy: PIL hands out a read-only buffer)


def write_rgb(path, arr):
    from PIL import Image
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    Image.fromarray(arr, mode="RGB").save(path)


def load_params(path):
    sd = torch.load(path, map_location="cpu")
    return sd["params"] if isinstance(sd, dict) and "params" in sd else sd     # inference_fdn_lolblur.py:28,31


def tile_arg(s):
    """--tile: 'off' -> None, 'auto' -> "auto", 'HxW' with both numbers positive multiples of 32 -> (H, W)"""
    if s in ("off", "auto"):
        return None if s == "off" else s
    try:
        h, w = (int(v) for v in s.lower().split("x"))
    except ValueError:
        raise argparse.ArgumentTypeError(f"{s!r} is not HxW, auto or off")
    if h <= 0 or w <= 0 or h % 32 or w % 32:
        raise argparse.ArgumentTypeError(f"{s!r}: both tile sizes must be positive multiples of 32")
    return h, w


def add_tile_args(ap, ratio_default="frame"):
    """--tile / --tile-overlap / --tile-blend, and --tile-ratio unless ratio_default is None (a driver whose ratio is fixed)"""
    ap.add_argument("--tile", type=tile_arg, default=None, metavar="HxW|auto|off",
                    help="run frames as overlapping tiles of this size (multiples of 32), merged by averaging; auto: 736x1280 tiles for "
                         "frames above 1088x1920 pixels only; default off")
    ap.add_argument("--tile-overlap", type=int, default=0, metavar="N",
                    help="least number of pixels neighbouring tiles share (default 0: the reference's rule, no overlap when a side is a "
                         "multiple of the tile)")
    ap.add_argument("--tile-blend", choices=("average", "feather"), default="average",
                    help="how overlapping tiles are merged: the reference's uniform average (default), or feather: linear ramps across "
                         "each overlap, so no step where a tile's coverage ends (give it room with --tile-overlap)")
    if ratio_default is not None:
        ap.add_argument("--tile-ratio", choices=("frame", "tile"), default=ratio_default,
                        help=f"take the ratio from the whole frame or from each tile (default {ratio_default})")


def add_ensemble_arg(ap):
    """--ensemble: the number of flipped / transposed copies per frame, fdn_hip.ensemble.MASKS"""
    ap.add_argument("--ensemble", type=int, choices=(1, 2, 4, 8), default=1,
                    help="geometric self-ensemble: run FDN on this many flipped / transposed copies of every frame (or tile) and average "
                         "the results mapped back: 2 = plus the column mirror, 4 = all mirrors, 8 = all mirrors and transpositions; "
                         "default 1 (off)")


def bracket_arg(s):
    """--bracket: 'EV[,EV...]' -> a tuple of 1 to 16 distinct finite exposure stops (fdn_hip.fusion.check_bracket)"""
    from fdn_hip.fusion import check_bracket
    try:
        return check_bracket([float(v) for v in s.split(",")])
    except ValueError as e:
        raise argparse.ArgumentTypeError(f"{s!r}: {e}")


def fusion_weights_arg(s):
    """--fusion-weights: 'C,S,E' -> three finite exponents >= 0 (fdn_hip.fusion.check_exponents)"""
    from fdn_hip.fusion import check_exponents
    try:
        return check_exponents([float(v) for v in s.split(",")])
    except ValueError as e:
        raise argparse.ArgumentTypeError(f"{s!r}: {e}")


def ratio_value(s):
    """--ratio VALUE: a finite float"""
    try:
        v = float(s)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{s!r} is not a number")
    if v != v or v in (float("inf"), float("-inf")):
        raise argparse.ArgumentTypeError(f"{s!r} is not finite")
    return v


def glue_bracket(argv):
    """argv (None: the process's) with '--bracket' and the word after it joined by '=': argparse takes a value that begins with '-'
    and is not a plain number, such as -1,0,1, for an option"""
    argv = list(sys.argv[1:] if argv is None else argv)
    out = []
    while argv:
        tok = argv.pop(0)
        out.append(tok + "=" + argv.pop(0) if tok == "--bracket" and argv else tok)
    return out


def add_fusion_args(ap):
    """--bracket / --fusion-weights: exposure fusion of every frame's renderings at a bracket of ratios (fdn_hip.fusion)"""
    ap.add_argument("--bracket", type=bracket_arg, default=None, metavar="EV[,EV...]",
                    help="render every frame at its ratio times 2^-EV for each of these 1 to 16 exposure stops (positive: brighter), for "
                         "example -1,0,1, and fuse the renderings into one locally exposed frame; default off")
    ap.add_argument("--fusion-weights", type=fusion_weights_arg, default=(1.0, 1.0, 1.0), metavar="C,S,E",
                    help="with --bracket: the exponents of contrast, saturation and well-exposedness in the fusion's weights (default 1,1,1)")


_hinted = False


def hint_large_frame(tile, h, w):
    """one line on stderr, once per run, when an untiled frame is larger than the whole-frame path is tested at"""
    global _hinted
    from fdn_hip.harness import padded_size
    from fdn_hip.tiling import WHOLE_FRAME_MAX_PIXELS
    H, W = padded_size(h, w)
    if tile is None and not _hinted and H * W > WHOLE_FRAME_MAX_PIXELS:
        _hinted = True
        print(f"note: a {h}x{w} frame is larger than a whole-frame forward is tested at (1088x1920 padded); --tile auto runs it in tiles",
              file=sys.stderr)


_seam_hinted = False


def hint_hard_seam(tile, blend, overlap, h, w):
    """one line on stderr, once per run, when --tile-blend feather meets a frame axis whose neighbouring tiles share no pixel (a side that
    is a multiple of the tile, with overlap 0): nothing to ramp across, the seam stays hard"""
    global _seam_hinted
    from fdn_hip.harness import resolve_tile
    from fdn_hip.tiling import effective_crop, tile_origins
    if blend != "feather" or _seam_hinted or tile is None:
        return
    crop = resolve_tile(tile, h, w)
    if crop is None or h < 32 or w < 32:
        return
    ch, cw = effective_crop(h, w, *crop)
    idx = tile_origins(h, w, ch, cw, overlap)
    for name, org, c in (("rows", sorted({i for i, _ in idx}), ch), ("columns", sorted({j for _, j in idx}), cw)):
        if any(a + c <= b for a, b in zip(org, org[1:])):
            _seam_hinted = True
            print(f"note: --tile-blend feather has no overlap to blend across along the {name} of a {h}x{w} frame cut into {ch}x{cw} tiles: "
                  "that seam stays hard; --tile-overlap N makes neighbouring tiles share at least N pixels", file=sys.stderr)
            return


def parse_driver_args(doc, fdn_keys="FDN checkpoint ({'params': state_dict}, 1503 keys)", argv=None):
    """the command line of the LOL-Blur and LOL-v1 drivers -> (parser, namespace)"""
    ap = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--fdn", required=True, help=fdn_keys)
    ap.add_argument("--lpnet", default=None, help="LPNet checkpoint (292 keys); needed unless --ratio is given")
    ap.add_argument("--ratio", type=ratio_value, default=None, metavar="VALUE",
                    help="feed FDN this ratio for every frame instead of LPNet's (a smaller ratio is brighter)")
    ap.add_argument("--input", required=True, help="glob of input frames")
    ap.add_argument("--output", required=True, help="output directory")
    ap.add_argument("--input-root", default=None,
                    help="directory the output tree mirrors: a frame <input-root>/0256/0089.png is written to <output>/0256/0089.png "
                         "(the reference keeps the LOL-Blur sequence folders the same way, inference_fdn_lolblur.py:44-45,73); "
                         "default: the common parent directory of all input frames")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--device", default="cuda:0")
    add_tile_args(ap)
    add_ensemble_arg(ap)
    add_fusion_args(ap)
    a = ap.parse_args(glue_bracket(argv))
    if a.ratio is None and not a.lpnet:
        ap.error("--lpnet is needed unless --ratio VALUE is given")
    return ap, a


def run_driver(doc, build_models, ratio_mode="lolblur", fdn_keys="FDN checkpoint ({'params': state_dict}, 1503 keys)"):
    """The directory walk shared by the LOL-Blur and LOL-v1 drivers: build_models() -> (FDN-like module, LPNet module) on the CPU,
    ratio_mode as fdn_hip.harness.enhance_u8 takes it."""
    ap, a = parse_driver_args(doc, fdn_keys)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1 and a.ensemble > 1:
        ap.error("--ensemble above 1 runs on one GPU only: the sharded tile server takes one tile shape")
    if world > 1 and a.tile is None:
        ap.error("WORLD_SIZE > 1 needs --tile: the ranks share the tiles of one frame; sharding whole frames by file is not supported")

    from fdn_hip import tiling
    from fdn_hip.harness import enhance_frame_tiled, enhance_u8, resolve_tile

    dist = None
    dev = torch.device(a.device)
    if world > 1:
        import torch.distributed as dist
        dev = torch.device("cuda", int(os.environ["LOCAL_RANK"]))
    torch.cuda.set_device(dev)
    if dist is not None:
        dist.init_process_group("nccl")
    net, lp = build_models()
    net = net.to(dev).eval()
    net.load_state_dict(load_params(a.fdn), strict=True)
    if a.ratio is None:
        lp = lp.to(dev).eval()
        lp.load_state_dict(load_params(a.lpnet), strict=True)
    else:
        lp, ratio_mode = None, "fixed"

    tile_kw = dict(ratio_from=a.tile_ratio, overlap=a.tile_overlap, batch=a.batch, blend=a.tile_blend)
    if a.bracket is not None:                                            # without the option every call is what it was
        tile_kw.update(bracket=a.bracket, fusion=a.fusion_weights)

    def fixed(n):
        """the ratio keyword of a call on n frames: --ratio for each of them, or nothing"""
        return {} if a.ratio is None else {"ratio": torch.full((n, 1), a.ratio, dtype=torch.float32, device=dev)}

    def serve(tiles, ratio):
        return tiling.run_tiles(net, tiles, ratio, a.batch)

    if dist is not None and dist.get_rank() != 0:
        tiling.serve_tiles(dist, serve, dev)                              # until rank 0 has written its last frame
        dist.destroy_process_group()
        return

    def enhance(batch):
        """uint8 [B,h,w,3] -> uint8 [B,h,w,3]; with more than one rank the tiles of each frame go through all of them"""
        h, w = batch.shape[1:3]
        hint_large_frame(a.tile, h, w)
        hint_hard_seam(a.tile, a.tile_blend, a.tile_overlap, h, w)
        if dist is None:
            return enhance_u8(net, lp, batch, bgr=False, ratio_mode=ratio_mode, tile=a.tile, ensemble=a.ensemble, **fixed(len(batch)),
                              **tile_kw)
        if resolve_tile(a.tile, h, w) is None:
            return enhance_u8(net, lp, batch, bgr=False, ratio_mode=ratio_mode, **fixed(len(batch)),
                              **({k: v for k, v in tile_kw.items() if k in ("bracket", "fusion")}))
        return torch.stack([enhance_frame_tiled(net, lp, img, a.tile, bgr=False, ratio_mode=ratio_mode, **fixed(1),
                                                run=lambda t, r: tiling.run_tiles_root(dist, serve, t, r), **tile_kw)[0] for img in batch])

    try:
        walk(a, dev, enhance)
    finally:
        if dist is not None:
            tiling.end_serving(dist)
            dist.destroy_process_group()


def walk(a, dev, enhance):
    """decode -> enhance(uint8 batch on the device) -> encode over the frames of a.input"""
    paths = sorted(glob.glob(a.input))
    if not paths:
        raise SystemExit(f"no input frames match {a.input}")
    root = a.input_root or os.path.commonpath([os.path.dirname(os.path.abspath(p)) for p in paths])
    dest = {p: os.path.join(a.output, os.path.relpath(os.path.abspath(p), root)) for p in paths}
    if any(d.startswith("..") for d in (os.path.relpath(v, a.output) for v in dest.values())):
        raise SystemExit(f"--input-root {root} does not contain every input frame")
    if len(set(dest.values())) != len(paths):                              # never let two frames race for one output file
        raise SystemExit("two input frames map to the same output path; pass an --input-root above both")
    with ThreadPoolExecutor(max_workers=4) as pool:
        decoded = pool.map(read_rgb, paths)                               # decode runs ahead of the GPU
        pending, writers = [], []

        def flush():
            if not pending:
                return
            batch = torch.from_numpy(np.stack([im for _, im in pending])).to(dev, non_blocking=True)
            out = enhance(batch).cpu().numpy()
            for (p, _), o in zip(pending, out):
                writers.append(pool.submit(write_rgb, dest[p], o))
            pending.clear()

        for p, im in zip(paths, decoded):
            if pending and (pending[0][1].shape != im.shape or len(pending) == a.batch):
                flush()
            pending.append((p, im))
        flush()
        for w in writers:
            w.result()
    print(f"{len(paths)} frames -> {a.output}")


def main():
    def build():
        from basicsr.models.archs.FDN_arch import FDN
        from basicsr.models.archs.LPNet_arch import I_predict_net
        return FDN(), I_predict_net()
    run_driver(__doc__, build)


if __name__ == "__main__":
    main()
