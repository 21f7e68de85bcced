"""Tiled inference on the GPU: the reference's mechanism for images larger than a forward can take
(ImageRestorationModel.grids / grids_inverse, basicsr/models/image_restoration_model.py:261-339, enabled by
`val.grids` with `crop_size_h/w`, :737-743).  Tiles overlap by an adaptive step, run through the network as a batch
and are averaged where they overlap - the result differs from an untiled forward (FDN's FFTs are global), so this is a
feature of the reference being mirrored, not an optimisation.  scale = 1 (restoration, `opt['scale']`).

blend="feather" is this project's own option beside that average: the tiles are weighted with linear ramps across their overlaps
(feather_weights), so the merged frame has no step where one tile's coverage ends.  The default everywhere is the reference's average.
"""
import math

import numpy as np
import torch

from . import FdnHipError, check, dev_as, lib, ptr, stream

F32, U8 = torch.float32, torch.uint8


# The largest reflect-padded frame a whole-frame forward is pinned at by the GPU suite (tests/test_gpu_configs.py, BASELINE.json
# configs[2]: 1088 x 1920).  Above it nothing is tested, and from about 3 Mpx one per-image tensor of the dim-32 network (172 planes)
# passes the 2 GiB that csrc/buffer_io.hpp can address ("Limits") - so auto_tile() tiles every frame above this size.
WHOLE_FRAME_MAX_PIXELS = 1088 * 1920
AUTO_TILE = (736, 1280)         # the padded 720p frame: the flagship shape, compile-time FFT plans on every level


def _tile_count(n, c, v):
    return 1 if c >= n else -(-(n - v) // (c - v))


def tile_origins(h, w, crop_h, crop_w, overlap=0):
    """Origins (i, j) of the tiles, image_restoration_model.py:278-309.  overlap = 0 is the reference's rule, which leaves no overlap at
    all (hard seams in the merge) whenever a side is a multiple of the crop; overlap = v asks for enough tiles per axis that neighbours
    share at least v pixels: ceil((n - v) / (c - v)) instead of ceil(n / c).  Step and walk are the reference's either way."""
    if crop_h > h or crop_w > w or crop_h <= 0 or crop_w <= 0:
        raise FdnHipError(f"crop {crop_h}x{crop_w} does not fit the image {h}x{w}")
    if not 0 <= overlap < min(crop_h, crop_w):
        raise FdnHipError(f"overlap {overlap} must be in [0, crop) for the crop {crop_h}x{crop_w}")
    num_row, num_col = _tile_count(h, crop_h, overlap), _tile_count(w, crop_w, overlap)
    step_j = crop_w if num_col == 1 else math.ceil((w - crop_w) / (num_col - 1) - 1e-8)
    step_i = crop_h if num_row == 1 else math.ceil((h - crop_h) / (num_row - 1) - 1e-8)
    idx = []
    i, last_i = 0, False
    while i < h and not last_i:
        j = 0
        if i + crop_h >= h:
            i, last_i = h - crop_h, True
        last_j = False
        while j < w and not last_j:
            if j + crop_w >= w:
                j, last_j = w - crop_w, True
            idx.append((i, j))
            j += step_j
        i += step_i
    return idx


def auto_tile(h, w):
    """The tile for an h x w frame under --tile auto: None (run it whole) while the reflect-padded frame has at most
    WHOLE_FRAME_MAX_PIXELS pixels, else the 736 x 1280 tile clipped to the frame's whole 32-pixel blocks."""
    H, W = h + (32 - h % 32) % 32, w + (32 - w % 32) % 32
    if H * W <= WHOLE_FRAME_MAX_PIXELS:
        return None
    return min(AUTO_TILE[0], h // 32 * 32), min(AUTO_TILE[1], w // 32 * 32)


def effective_crop(h, w, crop_h, crop_w):
    """The tile split_u8 / merge_u8 use for an h x w frame: per axis min(crop, whole 32-pixel blocks of the frame) - tiles are cut from
    the unpadded frame and the network takes multiples of 32 only."""
    if crop_h <= 0 or crop_w <= 0 or crop_h % 32 or crop_w % 32:
        raise FdnHipError(f"tile sizes must be positive multiples of 32 (three levels x 8x8 patches), got {crop_h}x{crop_w}")
    if h < 32 or w < 32:
        raise FdnHipError(f"a {h}x{w} frame has a side under 32 pixels and cannot be tiled: run it on the untiled path (tile=None), "
                          "which reflect-pads it")
    return min(crop_h, h // 32 * 32), min(crop_w, w // 32 * 32)


def split(x, crop_h, crop_w, overlap=0):
    """grids(): x (1,C,h,w) -> (tiles (T,C,crop_h,crop_w), origins tensor int32 [T,2] on the device)."""
    if x.dim() != 4 or x.shape[0] != 1:
        raise FdnHipError("tiled inference takes one image at a time (the reference asserts b == 1, :265)")
    _, C, h, w = x.shape
    idx = tile_origins(h, w, crop_h, crop_w, overlap)
    ij = torch.tensor(idx, dtype=torch.int32, device=x.device)
    tiles = torch.empty((len(idx), C, crop_h, crop_w), device=x.device, dtype=torch.float32)
    check(lib().fdn_tiles_gather(dev_as(x, F32, "x"), dev_as(tiles, F32, "tiles"), ptr(ij), len(idx), C, h, w, crop_h,
                                 crop_w, stream()), "fdn_tiles_gather")
    return tiles, ij


BLENDS = ("average", "feather")


def check_blend(blend):
    if blend not in BLENDS:
        raise ValueError(f"blend {blend!r}: 'average' (the reference's grids_inverse) or 'feather'")
    return blend


def _axis_ramps(origins, c):
    """{origin: float64 [c]} for the tiles of length c along one axis: a linear ramp across the pixels shared with the previous tile and
    with the next one, sampled at pixel centres, 1 elsewhere; where both ramps reach a pixel the smaller one holds"""
    o = sorted(set(origins))
    d = np.arange(c, dtype=np.float64)
    ramps = {}
    for k, ok in enumerate(o):
        lo = max(0, o[k - 1] + c - ok) if k > 0 else 0
        hi = max(0, ok + c - o[k + 1]) if k + 1 < len(o) else 0
        wgt = np.ones(c, dtype=np.float64)
        if lo > 0:
            wgt[:lo] = np.minimum(wgt[:lo], (d[:lo] + 0.5) / lo)
        if hi > 0:
            wgt[c - hi:] = np.minimum(wgt[c - hi:], (c - d[c - hi:] - 0.5) / hi)
        ramps[ok] = wgt
    return ramps


def feather_weights(idx, ch, cw):
    """The weights of the feathered merge for the origins tile_origins returns -> (wy float32 [T][ch], wx float32 [T][cw]) on the CPU; tile
    t weighs its pixel (dy, dx) with wy[t][dy] * wx[t][dx].  Per axis, with the unique origins sorted, a tile ramps up over the
    lo = o[k-1] + c - o[k] pixels it shares with its predecessor, w(d) = (d + 0.5) / lo, and down over the hi = o[k] + c - o[k+1] pixels
    it shares with its successor, w(d) = (c - d - 0.5) / hi; the weight is 1 elsewhere, and on a side at the frame's border or without
    an overlapping neighbour.  Every weight is positive, and the ramps of two tiles that alone share a band sum to 1.  float64, rounded
    once to float32."""
    idx = [(int(i), int(j)) for i, j in idx]
    rows, cols = sorted({i for i, _ in idx}), sorted({j for _, j in idx})
    if not idx or len(idx) != len(rows) * len(cols) or set(idx) != {(i, j) for i in rows for j in cols}:
        raise FdnHipError(f"feather_weights needs the full grid of origins that tile_origins returns, got {len(idx)} origins over "
                          f"{len(rows)} rows and {len(cols)} columns")
    if ch <= 0 or cw <= 0:
        raise FdnHipError(f"tile {ch}x{cw} must be positive")
    ry, rx = _axis_ramps(rows, ch), _axis_ramps(cols, cw)
    wy = np.stack([ry[i] for i, _ in idx]).astype(np.float32)
    wx = np.stack([rx[j] for _, j in idx]).astype(np.float32)
    return torch.from_numpy(wy), torch.from_numpy(wx)


def _feather_on_device(ij, ch, cw):
    wy, wx = feather_weights(ij.cpu().tolist(), ch, cw)
    return wy.to(ij.device).contiguous(), wx.to(ij.device).contiguous()


def merge(outs, ij, h, w, blend="average"):
    """grids_inverse(): tiles (T,C,ch,cw) + origins -> (1,C,h,w), overlaps averaged (blend "average", the reference) or weighted with
    feather_weights ("feather": no step where a tile's coverage ends)."""
    check_blend(blend)
    T, C, ch, cw = outs.shape
    out = torch.empty((1, C, h, w), device=outs.device, dtype=torch.float32)
    if blend == "feather":
        if tuple(ij.shape) != (T, 2):
            raise FdnHipError(f"cannot merge tiles {tuple(outs.shape)} with origins {tuple(ij.shape)}")
        wy, wx = _feather_on_device(ij, ch, cw)
        check(lib().fdn_tiles_merge_w(dev_as(outs, F32, "outs"), dev_as(out, F32, "out"), ptr(ij), dev_as(wy, F32, "wy"), dev_as(wx, F32, "wx"),
                                      T, C, h, w, ch, cw, stream()), "fdn_tiles_merge_w")
        return out
    check(lib().fdn_tiles_merge(dev_as(outs, F32, "outs"), dev_as(out, F32, "out"), ptr(ij), T, C, h, w, ch, cw, stream()),
          "fdn_tiles_merge")
    return out


def split_u8(img_u8, crop_h, crop_w, bgr=True, overlap=0):
    """grids() straight from the uint8 frame [h,w,3]: -> (tiles (T,3,ch,cw) fp32 RGB in [0,1], origins int32 [T,2] on the device), with
    (ch, cw) = effective_crop.  Bit for bit harness.preprocess without padding followed by split()."""
    if img_u8.dim() != 3 or img_u8.shape[-1] != 3:
        raise FdnHipError(f"expected one uint8 frame [h,w,3], got {tuple(img_u8.shape)}")
    h, w, _ = img_u8.shape
    ch, cw = effective_crop(h, w, crop_h, crop_w)
    idx = tile_origins(h, w, ch, cw, overlap)
    src = dev_as(img_u8, U8, "img")
    ij = torch.tensor(idx, dtype=torch.int32, device=img_u8.device)
    tiles = torch.empty((len(idx), 3, ch, cw), device=img_u8.device, dtype=torch.float32)
    check(lib().fdn_tiles_gather_u8(src, dev_as(tiles, F32, "tiles"), ptr(ij), len(idx), h, w, ch, cw, int(bool(bgr)),
                                    stream()), "fdn_tiles_gather_u8")
    return tiles, ij


def merge_u8(outs, ij, h, w, bgr=True, blend="average"):
    """grids_inverse() straight to the uint8 frame: tiles (T,3,ch,cw) + origins -> uint8 [h,w,3], overlaps averaged or feathered (blend,
    as merge takes it), then clamp(0,1), *255, round half to even.  Bit for bit merge() followed by harness.postprocess."""
    check_blend(blend)
    T, C, ch, cw = outs.shape
    if C != 3 or ch > h or cw > w or tuple(ij.shape) != (T, 2) or ij.dtype != torch.int32 or not ij.is_cuda:
        raise FdnHipError(f"cannot merge tiles {tuple(outs.shape)} with origins {tuple(ij.shape)} into a {h}x{w} frame")
    out = torch.empty((h, w, 3), device=outs.device, dtype=torch.uint8)
    if blend == "feather":
        wy, wx = _feather_on_device(ij, ch, cw)
        check(lib().fdn_tiles_merge_w_u8(dev_as(outs, F32, "outs"), dev_as(out, U8, "out"), ptr(ij), dev_as(wy, F32, "wy"), dev_as(wx, F32, "wx"),
                                         T, h, w, ch, cw, int(bool(bgr)), stream()), "fdn_tiles_merge_w_u8")
        return out
    check(lib().fdn_tiles_merge_u8(dev_as(outs, F32, "outs"), dev_as(out, U8, "out"), ptr(ij), T, h, w, ch, cw, int(bool(bgr)),
                                   stream()), "fdn_tiles_merge_u8")
    return out


@torch.no_grad()
def run_tiles(net, tiles, ratio, batch=8, ensemble=1):
    """FDN on tiles (T,3,ch,cw) with ratio (T,1), `batch` tiles per forward (the last forward may take fewer) -> outs (T,3,ch,cw).
    ensemble 2, 4 or 8: every tile goes through FDN in that many flipped / transposed copies with its own ratio, and outs holds their
    average (fdn_hip.ensemble: fdn_d4_apply -> forwards -> fdn_d4_mean)."""
    from .ensemble import check_ensemble
    check_ensemble(ensemble)
    T = tiles.shape[0]
    if tuple(ratio.shape) != (T, 1):
        raise FdnHipError(f"run_tiles needs ratio [{T},1], got {tuple(ratio.shape)}")
    if batch < 1:
        raise FdnHipError(f"batch must be at least 1, got {batch}")
    ratio = ratio.to(device=tiles.device, dtype=torch.float32)
    if ensemble != 1:
        from . import ensemble as ens
        res_a, res_b, mask = ens.forward_ensemble(net, tiles.contiguous(), ratio, ensemble, batch)
        return ens.mean(res_a, res_b, mask, tiles.shape[2], tiles.shape[3])
    outs = torch.empty_like(tiles)
    for s in range(0, T, batch):
        t = tiles[s:s + batch]
        outs[s:s + batch] = net(t, ratio_i=ratio[s:s + batch].contiguous(), device=t.device)[0]
    return outs


def run_tiles_sharded(dist, forward, T, sample_like, tiles=None, ratio=None, root=0):
    """The tiles of one frame over the ranks of a node: the root holds tiles [T,...] and ratio [T,1] (None elsewhere), both go out with
    sharding.scatter_uneven, every rank runs forward(its tiles, its ratio) - not called on a rank that received no tile - and
    gather_uneven returns outs [T,...] on the root, None elsewhere.  forward keeps the tiles' trailing shape and dtype (FDN does), which
    is what a rank without a tile contributes.  sample_like: one tile [1,...] on this rank's device.  The collectives are the blocking
    ones of fdn_hip.sharding, strictly serial with the forward."""
    from . import sharding
    my_tiles = sharding.scatter_uneven(dist, T, sample_like, tiles, src=root)
    my_ratio = sharding.scatter_uneven(dist, T, sample_like.new_empty((1, 1)), ratio, src=root)
    out = forward(my_tiles, my_ratio) if my_tiles.shape[0] else my_tiles
    return sharding.gather_uneven(dist, out, T, dst=root)


def serve_tiles(dist, forward, device, root=0):
    """What every rank but the root does while the root walks the frames: wait for the root's (T, ch, cw), take part in that frame's
    run_tiles_sharded, and return when the root sends None (end_serving)."""
    while True:
        desc = [None]
        dist.broadcast_object_list(desc, src=root)
        if desc[0] is None:
            return
        T, ch, cw = desc[0]
        run_tiles_sharded(dist, forward, T, torch.empty((1, 3, ch, cw), device=device, dtype=torch.float32), root=root)


def run_tiles_root(dist, forward, tiles, ratio, root=0):
    """The root's side of serve_tiles for one frame: announce (T, ch, cw), then run_tiles_sharded -> outs [T,3,ch,cw]."""
    T, _, ch, cw = tiles.shape
    dist.broadcast_object_list([(T, ch, cw)], src=root)
    return run_tiles_sharded(dist, forward, T, tiles[:1], tiles, ratio.to(device=tiles.device, dtype=torch.float32).contiguous(), root=root)


def end_serving(dist, root=0):
    dist.broadcast_object_list([None], src=root)


@torch.no_grad()
def forward_tiled(net, lpnet, x, crop_h, crop_w, batch=8, ratio=None, overlap=0, blend="average", ensemble=1):
    """LPNet -> FDN on overlapping tiles of one padded image (crop sizes multiples of 32), merged like the reference.  ratio: [T,1]
    (one per tile) or [1,1] (one for the frame) feeds FDN instead of LPNet's per-tile prediction; overlap as tile_origins takes it,
    blend as merge takes it, ensemble as run_tiles takes it (LPNet's prediction is then taken from the untransformed tile)."""
    from .ensemble import check_ensemble
    check_blend(blend)
    check_ensemble(ensemble)
    if crop_h % 32 or crop_w % 32:
        raise FdnHipError("tile sizes must be multiples of 32 (three levels x 8x8 patches)")
    tiles, ij = split(x.contiguous(), crop_h, crop_w, overlap)
    if ratio is not None:
        if ratio.dim() != 2 or ratio.shape[1] != 1 or ratio.shape[0] not in (1, tiles.shape[0]):
            raise FdnHipError(f"ratio must be [1,1] or [{tiles.shape[0]},1], got {tuple(ratio.shape)}")
        return merge(run_tiles(net, tiles, ratio.expand(tiles.shape[0], 1), batch, ensemble), ij, x.shape[2], x.shape[3], blend)
    if ensemble != 1:
        ratio = torch.cat([lpnet(tiles[s:s + batch]) for s in range(0, tiles.shape[0], batch)])
        return merge(run_tiles(net, tiles, ratio, batch, ensemble), ij, x.shape[2], x.shape[3], blend)
    outs = torch.empty_like(tiles)
    for s in range(0, tiles.shape[0], batch):
        t = tiles[s:s + batch]
        outs[s:s + batch] = net(t, ratio_i=lpnet(t), device=t.device)[0]
    return merge(outs, ij, x.shape[2], x.shape[3], blend)
