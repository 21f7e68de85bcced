"""The step either side of the LPNet -> FDN forward, on the GPU.

Mirrors what inference_fdn_lolblur.py:47-75 does on the host with cv2 / numpy:

    img = cv2.imread(p).astype(np.float32) / 255.          # uint8 BGR HWC -> fp32
    img = img2tensor(img, bgr2rgb=True)[None]               # RGB CHW, batch 1        (img_util.py:9-33)
    img = F.pad(img, (0, w_n, 0, h_n), 'reflect')           # bottom/right to the x32 grid
    ratio = LPNet(img); result = FDN(img, ratio_i=ratio)[0]
    out = tensor2img(result[:, :, :h, :w], rgb2bgr=True)    # clamp, *255, round, uint8 BGR HWC (img_util.py:36-98)

here as two HIP kernels (fdn_pre_u8 / fdn_post_u8) around the drop-in modules, batched: B images of one size go
through one forward.  No CPU fallback: the uint8 tensors must live on the ROCm device.

validate_u8 is the same walk with a ground truth beside the input, as the reference's validation does it
(basicsr/models/image_restoration_model.py:578-586, :650-658, :746-748, :844-848): the ratio from the ground truth (gt_ratio), and
PSNR / SSIM of the uint8 result against the uint8 ground truth.

With `tile`, a frame larger than one forward can take goes uint8 -> tiling.split_u8 -> tiling.run_tiles -> tiling.merge_u8 -> uint8 (the
reference's val.grids, image_restoration_model.py:261-339, :737-743), one frame at a time; no fp32 frame exists except the one a
frame-level ratio is taken from.  blend="feather" merges the tiles with ramps across their overlaps instead of the reference's average.

Video frames (no reference counterpart): preprocess_yuv420 / postprocess_yuv420 / enhance_yuv420 are the same walk between Y'CbCr 4:2:0
frames as a decoder hands them out (VideoFormat: yuv420p, nv12, yuv420p10le) and the same forward, through fdn_pre_yuv420 /
fdn_post_yuv420 (include/fdn_video.h): codec samples -> fp32 -> codec samples, rounded once.  enhance_yuv420(temporal=RatioFilter) filters
the ratio across the frames of a stream (fdn_hip.temporal, include/fdn_temporal.h).

ensemble = 2, 4 or 8 (enhance_u8, validate_u8, enhance_frame_tiled; no reference counterpart) is the geometric self-ensemble of
fdn_hip.ensemble: FDN runs on that many flipped / transposed copies of each frame - or, tiled, of each tile - with the ratio of the
untransformed frame or tile, and the results, mapped back, are averaged.  ensemble = 1 is the code path without the keyword.

bracket = a tuple of exposure stops (enhance_u8, validate_u8, enhance_frame_tiled; no reference counterpart) renders every frame at the
ratios fdn_hip.fusion.bracket_ratios makes of the one the call without a bracket would feed, and fuses the renderings into one locally
exposed frame (fdn_hip.fusion, render_ratios).  bracket = None is the code path without the keyword.
"""
import ctypes
from dataclasses import dataclass

import torch

from . import lib, check, dev_as, stream, FdnHipError


def padded_size(h, w, multiple=32):
    """inference_fdn_lolblur.py:57-59: pad bottom/right up to the next multiple of 32."""
    return h + (multiple - h % multiple) % multiple, w + (multiple - w % multiple) % multiple


def preprocess(img_u8, bgr=True):
    """uint8 [B,h,w,3] (or [h,w,3]) on the GPU -> (fp32 [B,3,H,W] reflect-padded RGB in [0,1], h, w)."""
    if img_u8.dim() == 3:
        img_u8 = img_u8.unsqueeze(0)
    if img_u8.dim() != 4 or img_u8.shape[-1] != 3:
        raise FdnHipError(f"expected uint8 images [B,h,w,3], got {tuple(img_u8.shape)}")
    B, h, w, _ = img_u8.shape
    H, W = padded_size(h, w)
    if H - h >= h or W - w >= w:
        raise FdnHipError(f"reflect padding {h}x{w} -> {H}x{W} needs pad < size (F.pad raises the same way)")
    out = torch.empty((B, 3, H, W), device=img_u8.device, dtype=torch.float32)
    check(lib().fdn_pre_u8(dev_as(img_u8, torch.uint8, "img"), ctypes.c_void_p(out.data_ptr()), B, h, w, H, W, int(bool(bgr)), stream()),
          "fdn_pre_u8")
    return out, h, w


def postprocess(result, h, w, bgr=True):
    """fp32 [B,3,H,W] -> uint8 [B,h,w,3]: crop, clamp(0,1), *255, round half-to-even (numpy .round())."""
    if not result.is_cuda or result.dtype != torch.float32 or not result.is_contiguous() or result.dim() != 4:
        raise FdnHipError("result must be a contiguous float32 ROCm tensor [B,3,H,W]")
    B, C, H, W = result.shape
    if C != 3 or h > H or w > W:
        raise FdnHipError(f"cannot crop {h}x{w} out of {tuple(result.shape)}")
    out = torch.empty((B, h, w, 3), device=result.device, dtype=torch.uint8)
    check(lib().fdn_post_u8(ctypes.c_void_p(result.data_ptr()), dev_as(out, torch.uint8, "out"), B, h, w, H, W, int(bool(bgr)), stream()),
          "fdn_post_u8")
    return out


def lolv1_ratio(x, lp_ratio):
    """inference_fdn_lolv1.py:57-61: ratio_i = mean(Grayscale(padded input)) / LPNet(padded input).  The plane means
    come from fdn_global_avgpool; Grayscale is linear (0.2989 R + 0.587 G + 0.114 B), so its mean is the same
    combination of the three plane means ([B,3] values, combined on the device)."""
    return _gray_mean(x) / lp_ratio


def _gray_mean(x):
    """[B,3,H,W] R, G, B -> [B,1]: the mean of transforms.Grayscale's plane"""
    from . import ops
    m = ops.global_avgpool(x).reshape(x.shape[0], 3)
    return 0.2989 * m[:, 0:1] + 0.587 * m[:, 1:2] + 0.114 * m[:, 2:3]


def gt_ratio(x_lq, x_gt):
    """The ratio the reference's validation feeds FDN (image_restoration_model.py:650-654 with use_ratio, options/train/FDN.yml):
    mean(Grayscale(padded input)) / mean(Grayscale(padded ground truth)), both reflect-padded as :583-586 -> [B,1].  Built like
    lolv1_ratio on fdn_global_avgpool.  A ground truth whose gray mean is 0 has no ratio."""
    if x_lq.shape != x_gt.shape or x_lq.dim() != 4 or x_lq.shape[1] != 3:
        raise FdnHipError(f"gt_ratio needs two [B,3,H,W] tensors of one shape, got {tuple(x_lq.shape)} and {tuple(x_gt.shape)}")
    high = _gray_mean(x_gt)
    if bool((high == 0).any()):
        raise FdnHipError("gt_ratio: a ground-truth image has gray mean 0")
    return _gray_mean(x_lq) / high


def _frame_f32(img_u8, bgr):
    """uint8 [h,w,3] -> fp32 [1,3,h,w] RGB in [0,1], unpadded: fdn_tiles_gather_u8 with one tile the size of the frame"""
    h, w, _ = img_u8.shape
    ij = torch.zeros((1, 2), dtype=torch.int32, device=img_u8.device)
    out = torch.empty((1, 3, h, w), device=img_u8.device, dtype=torch.float32)
    check(lib().fdn_tiles_gather_u8(dev_as(img_u8, torch.uint8, "img"), ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ij.data_ptr()), 1,
                                    h, w, h, w, int(bool(bgr)), stream()), "fdn_tiles_gather_u8")
    return out


def resolve_tile(tile, h, w):
    """The `tile` keyword for an h x w frame -> None (the untiled path) or (crop_h, crop_w): "auto" is tiling.auto_tile."""
    from . import tiling
    if tile is None:
        return None
    if isinstance(tile, str):
        if tile != "auto":
            raise ValueError(f"tile {tile!r}: None, 'auto' or (crop_h, crop_w)")
        return tiling.auto_tile(h, w)
    crop_h, crop_w = tile
    return int(crop_h), int(crop_w)


def _per_tile(fn, tiles, batch):
    """fn on sub-batches of `batch` tiles, as the forward takes them -> [T,1]"""
    return torch.cat([fn(tiles[s:s + batch]) for s in range(0, tiles.shape[0], batch)])


def frame_ratio(lpnet, x, ratio_mode, x_gt=None):
    """The ratio [B,1] of reflect-padded fp32 frames x [B,3,H,W] as the untiled call feeds it: LPNet ("lolblur"), mean(gray) / LPNet
    ("lolv1") or gt_ratio against the padded ground truth x_gt ("gt")."""
    if ratio_mode == "gt":
        return gt_ratio(x, x_gt)
    if ratio_mode == "lolblur":
        return lpnet(x)
    return lolv1_ratio(x, lpnet(x))


def _tile_ratio(lpnet, tiles, ratio_mode, ratio_from, ratio, batch, frame, gt=None):
    """tile_ratio on fp32 frames, whatever they were converted from: frame() -> the reflect-padded fp32 frame [1,3,H,W]; gt, for ratio_mode
    "gt", a pair of such callables: the ground truth padded, and whole and unpadded."""
    if ratio_from not in ("frame", "tile"):
        raise ValueError(f"ratio_from {ratio_from!r}")
    T = tiles.shape[0]
    if ratio_mode == "fixed":
        if ratio is None or ratio.dim() != 2 or ratio.shape[1] != 1 or ratio.shape[0] not in (1, T):
            raise FdnHipError(f"ratio_mode 'fixed' on {T} tiles needs ratio [1,1] or [{T},1]")
        return ratio.to(device=tiles.device, dtype=torch.float32).expand(T, 1).contiguous()
    if ratio_mode == "gt" and gt is None:
        raise FdnHipError("ratio_mode 'gt' needs the ground-truth frame")
    if ratio_mode != "gt" and lpnet is None:
        raise FdnHipError(f"ratio_mode {ratio_mode!r} needs lpnet")
    if ratio_from == "frame":
        r = frame_ratio(lpnet, frame(), ratio_mode, gt[0]() if ratio_mode == "gt" else None)
        return r.expand(T, 1).contiguous()
    if ratio_mode == "lolblur":
        return _per_tile(lpnet, tiles, batch)
    if ratio_mode == "lolv1":
        return _per_tile(lambda t: lolv1_ratio(t, lpnet(t)), tiles, batch)
    high = _gray_mean(gt[1]())
    if bool((high == 0).any()):
        raise FdnHipError("gt_ratio: a ground-truth image has gray mean 0")
    return _per_tile(_gray_mean, tiles, batch) / high


def tile_ratio(lpnet, img_u8, tiles, ratio_mode, ratio_from, bgr=True, ratio=None, gt_u8=None, batch=8):
    """The ratio [T,1] that FDN takes on the tiles of one uint8 frame [h,w,3].
    ratio_from "frame": what the untiled call feeds - LPNet / mean(gray) / gt_ratio on the reflect-padded whole frame (LPNet's tensors are
    narrow, 16 planes at half resolution, so the whole frame fits) - for every tile alike.
    ratio_from "tile": the reference's val.grids semantics, where grids() has replaced the frame by its tiles before the ratio is taken
    (image_restoration_model.py:578-586, :650-654): LPNet / mean(gray) per tile; "gt" is mean(gray(tile)) / mean(gray(ground truth)) with
    the ground truth whole and unpadded (tiles are multiples of 32, so :583-586 pad nothing).
    "fixed": the caller's `ratio`, [1,1] for the frame or [T,1]."""
    gt = None if gt_u8 is None else (lambda: preprocess(gt_u8, bgr=bgr)[0], lambda: _frame_f32(gt_u8, bgr))
    return _tile_ratio(lpnet, tiles, ratio_mode, ratio_from, ratio, batch, lambda: preprocess(img_u8, bgr=bgr)[0], gt)


def _forward(net, lpnet, x, ratio_mode, ratio):
    """LPNet -> FDN on reflect-padded frames x [B,3,H,W] -> result [B,3,H,W]; ratio_mode / ratio as enhance_u8 takes them"""
    if ratio_mode == "fixed":
        if ratio is None or tuple(ratio.shape) != (x.shape[0], 1):
            raise FdnHipError(f"ratio_mode 'fixed' needs ratio [B,1] for B = {x.shape[0]}")
        return net(x, ratio_i=ratio.to(device=x.device, dtype=torch.float32).contiguous(), device=x.device)[0]
    if ratio_mode == "lolblur":
        from .pipeline import run
        return run(net, lpnet, x)                  # hipGraph replay for small frames, the eager forward otherwise
    return net(x, ratio_i=lolv1_ratio(x, lpnet(x)), device=x.device)[0]


@torch.no_grad()
def enhance_u8(net, lpnet, img_u8, bgr=True, ratio_mode="lolblur", ratio=None, tile=None, ratio_from="frame", overlap=0, batch=8,
               blend="average", ensemble=1, bracket=None, fusion=(1, 1, 1)):
    """uint8 in -> uint8 out through LPNet -> FDN (the body of the reference's per-image loop, batched).
    ratio_mode: "lolblur" feeds LPNet's prediction (inference_fdn_lolblur.py:69-71), "lolv1" feeds
    mean(gray)/prediction (inference_fdn_lolv1.py:57-62), "fixed" feeds the caller's `ratio` [B,1] and skips LPNet - the
    ratio sweep of inference_fdn_multi_r.py:78-84 (`ratio = ratio / ratio * i`).
    tile: None = every frame in one forward; (crop_h, crop_w), multiples of 32, or "auto" (tiling.auto_tile: only frames above
    tiling.WHOLE_FRAME_MAX_PIXELS) = frame by frame through enhance_frame_tiled, `batch` tiles per forward, neighbours sharing at least
    `overlap` pixels, the ratio taken from the whole frame or per tile (ratio_from, see tile_ratio; "fixed" then also takes [B,T,1]),
    the tiles merged by the reference's average or feathered (blend, see tiling.merge).  Without a tile, blend does nothing.
    ensemble: 1, 2, 4 or 8 copies of every frame (of every tile, with a tile) through FDN, averaged (fdn_hip.ensemble); the ratio is the
    one the call without `ensemble` feeds, taken once from the untransformed frame, and the forwards are eager, `batch` samples each.
    bracket: None, or 1 to 16 exposure stops, for example (-1, 0, 1): every frame is rendered at the ratios
    fdn_hip.fusion.bracket_ratios makes of the one the call without a bracket feeds (ratio * 2^-stop: a positive stop is brighter), `batch`
    stops per eager forward, and the renderings are fused over [:h, :w] (fdn_hip.fusion.fuse) before postprocess.  With a tile every stop
    is the merged fp32 frame of the tiled route, with an ensemble its fp32 mean.  fusion: the exponents of contrast, saturation and
    well-exposedness in the fusion's weights."""
    from .ensemble import check_ensemble
    from .tiling import check_blend
    if ratio_mode not in ("lolblur", "lolv1", "fixed"):
        raise ValueError(f"ratio_mode {ratio_mode!r}")
    check_blend(blend)
    check_ensemble(ensemble)
    if bracket is not None:
        from .fusion import check_bracket, check_exponents
        bracket, fusion = check_bracket(bracket), check_exponents(fusion)
    if img_u8.dim() == 3:
        img_u8 = img_u8.unsqueeze(0)
    if tile is not None and img_u8.dim() == 4 and resolve_tile(tile, img_u8.shape[1], img_u8.shape[2]) is not None:
        if ratio_mode == "fixed" and (ratio is None or ratio.shape[0] != img_u8.shape[0]):
            raise FdnHipError(f"ratio_mode 'fixed' needs ratio [B,1] or [B,T,1] for B = {img_u8.shape[0]}")
        return torch.stack([enhance_frame_tiled(net, lpnet, img_u8[b], tile, bgr=bgr, ratio_mode=ratio_mode, ratio_from=ratio_from,
                                                ratio=None if ratio is None else ratio[b].reshape(-1, 1), overlap=overlap, batch=batch,
                                                blend=blend, ensemble=ensemble, bracket=bracket, fusion=fusion)[0]
                            for b in range(img_u8.shape[0])])
    if bracket is not None:
        if ratio_mode == "fixed":
            if ratio is None or tuple(ratio.shape) != (img_u8.shape[0], 1):
                raise FdnHipError(f"ratio_mode 'fixed' needs ratio [B,1] for B = {img_u8.shape[0]}")
        else:
            ratio = frame_ratio(lpnet, preprocess(img_u8, bgr=bgr)[0], ratio_mode)
        return _bracket_u8(net, img_u8, ratio.to(device=img_u8.device), bracket, fusion, batch, ensemble, bgr)
    if ensemble != 1:
        if ratio_mode == "fixed":
            if ratio is None or tuple(ratio.shape) != (img_u8.shape[0], 1):
                raise FdnHipError(f"ratio_mode 'fixed' needs ratio [B,1] for B = {img_u8.shape[0]}")
        else:
            ratio = frame_ratio(lpnet, preprocess(img_u8, bgr=bgr)[0], ratio_mode)
        return _ensemble_u8(net, img_u8, ratio, ensemble, batch, img_u8.shape[1], img_u8.shape[2], bgr)
    x, h, w = preprocess(img_u8, bgr=bgr)
    return postprocess(_forward(net, lpnet, x, ratio_mode, ratio).contiguous(), h, w, bgr=bgr)


def _ensemble_u8(net, img_u8, ratio, ensemble, batch, h, w, bgr):
    """uint8 frames [B,h,w,3] + their ratio [B,1] -> uint8 [B,h,w,3] through the copies of fdn_hip.ensemble"""
    from . import ensemble as ens
    res_a, res_b, mask = ens.forward_ensemble(net, img_u8, ratio, ensemble, batch, bgr=bgr)
    return ens.post_u8(res_a, res_b, mask, h, w, bgr=bgr)


@torch.no_grad()
def render_ratios(net, img_u8, ratios, bgr=True, tile=None, overlap=0, batch=8, blend="average", ensemble=1, run=None, split=None):
    """One uint8 frame [h,w,3] through FDN at K ratios -> (fp32 [K,3,H,W], h, w) with H >= h, W >= w: the K renderings
    fdn_hip.fusion.fuse takes.  ratios: [K,1], or with a tile also [K,T,1], one row per tile.
    Untiled: the reflect-padded frame repeated, `batch` ratios per eager forward through the fixed-ratio route; the results keep their
    padding.  ensemble 2, 4 or 8: every rendering is the fp32 mean of that many copies (fdn_hip.ensemble.mean), h x w.
    tile (crop_h, crop_w): every rendering is the merged fp32 frame of the tiled route (tiling.run_tiles, or the caller's run(tiles, ratio)
    as enhance_frame_tiled takes it, then tiling.merge with `blend`), h x w.  split: the (tiles, origins) of tiling.split_u8 where the
    caller holds them already."""
    from . import tiling
    if img_u8.dim() != 3 or img_u8.shape[-1] != 3:
        raise FdnHipError(f"expected one uint8 frame [h,w,3], got {tuple(img_u8.shape)}")
    if batch < 1:
        raise FdnHipError(f"batch must be at least 1, got {batch}")
    h, w, _ = img_u8.shape
    K = ratios.shape[0]
    ratios = ratios.to(device=img_u8.device, dtype=torch.float32)
    if tile is not None:
        tiles, ij = split if split is not None else tiling.split_u8(img_u8, tile[0], tile[1], bgr=bgr, overlap=overlap)
        T = tiles.shape[0]
        if ratios.dim() == 2:
            ratios = ratios.reshape(K, 1, 1).expand(K, T, 1)
        if tuple(ratios.shape) != (K, T, 1):
            raise FdnHipError(f"render_ratios on {T} tiles needs ratios [K,1] or [K,{T},1], got {tuple(ratios.shape)}")
        frames = []
        for k in range(K):
            r = ratios[k].contiguous()
            outs = tiling.run_tiles(net, tiles, r, batch, ensemble=ensemble) if run is None else run(tiles, r)
            frames.append(tiling.merge(outs, ij, h, w, blend))
        return torch.cat(frames), h, w
    if ratios.dim() != 2 or ratios.shape[1] != 1:
        raise FdnHipError(f"render_ratios needs ratios [K,1], got {tuple(ratios.shape)}")
    if ensemble != 1:
        from . import ensemble as ens
        one = img_u8.unsqueeze(0)
        return torch.cat([ens.mean(*ens.forward_ensemble(net, one, ratios[k:k + 1], ensemble, batch, bgr=bgr), h, w) for k in range(K)]), h, w
    x = preprocess(img_u8, bgr=bgr)[0]
    frames = torch.empty((K,) + tuple(x.shape[1:]), device=x.device, dtype=torch.float32)
    for s in range(0, K, batch):
        n = min(batch, K - s)
        frames[s:s + n] = _forward(net, None, x.expand(n, -1, -1, -1).contiguous(), "fixed", ratios[s:s + n])
    return frames, h, w


def _bracket_u8(net, img_u8, ratio, bracket, fusion, batch, ensemble, bgr):
    """uint8 frames [B,h,w,3] + the ratio [B,1] the call without a bracket feeds -> uint8 [B,h,w,3]: frame by frame render_ratios at
    bracket_ratios of it, fusion.fuse, postprocess"""
    from . import fusion as fu
    rs = fu.bracket_ratios(ratio, bracket)
    out = []
    for b in range(img_u8.shape[0]):
        frames, h, w = render_ratios(net, img_u8[b], rs[b], bgr=bgr, batch=batch, ensemble=ensemble)
        out.append(postprocess(fu.fuse(frames, h, w, fusion).unsqueeze(0), h, w, bgr=bgr))
    return torch.cat(out)


@torch.no_grad()
def enhance_frame_tiled(net, lpnet, img_u8, tile, bgr=True, ratio_mode="lolblur", ratio_from="frame", ratio=None, gt_u8=None, overlap=0,
                        batch=8, run=None, blend="average", ensemble=1, bracket=None, fusion=(1, 1, 1)):
    """One uint8 frame [h,w,3] through the tiled route -> (uint8 [h,w,3], ratio [T,1]).  tile: (crop_h, crop_w) or "auto" (which must
    resolve to a tile here); ratio_mode / ratio_from / ratio / gt_u8 as tile_ratio takes them.  run(tiles, ratio) -> outs replaces
    tiling.run_tiles(net, tiles, ratio, batch) - the drivers pass the root's side of tiling.run_tiles_sharded.  blend: how the tiles are
    merged, "average" or "feather" (tiling.merge_u8); the merge runs here, on the root, whoever ran the tiles.  ensemble: copies of every
    tile through FDN with the tile's ratio, averaged before the merge (tiling.run_tiles); not with a caller's `run`, whose ranks are set
    up for one tile shape.  bracket / fusion as in enhance_u8: the tiles' ratio is taken as without a bracket (ratio_from unchanged), every
    stop scales it and runs the tiled route to a merged fp32 frame (a caller's `run` serves every stop), and the merged frames are fused;
    the ratio returned is the one without the stops."""
    from . import tiling
    from .ensemble import check_ensemble
    tiling.check_blend(blend)
    if check_ensemble(ensemble) != 1 and run is not None:
        raise ValueError("ensemble > 1 with a caller's run=: the sharded tile server takes one tile shape; run the ensemble on one GPU")
    if img_u8.dim() != 3 or img_u8.shape[-1] != 3:
        raise FdnHipError(f"expected one uint8 frame [h,w,3], got {tuple(img_u8.shape)}")
    h, w, _ = img_u8.shape
    crop = resolve_tile(tile, h, w)
    if crop is None:
        raise FdnHipError(f"a {h}x{w} frame needs no tile: run it on the untiled path")
    tiles, ij = tiling.split_u8(img_u8, crop[0], crop[1], bgr=bgr, overlap=overlap)
    r = tile_ratio(lpnet, img_u8, tiles, ratio_mode, ratio_from, bgr=bgr, ratio=ratio, gt_u8=gt_u8, batch=batch)
    if bracket is not None:
        from . import fusion as fu
        rs = fu.bracket_ratios(r, bracket).transpose(0, 1)                # [K,T,1]
        frames = render_ratios(net, img_u8, rs, bgr=bgr, tile=crop, overlap=overlap, batch=batch, blend=blend, ensemble=ensemble, run=run,
                               split=(tiles, ij))[0]
        return postprocess(fu.fuse(frames, h, w, fu.check_exponents(fusion)).unsqueeze(0), h, w, bgr=bgr)[0], r
    outs = tiling.run_tiles(net, tiles, r, batch, ensemble=ensemble) if run is None else run(tiles, r)
    return tiling.merge_u8(outs, ij, h, w, bgr=bgr, blend=blend), r


@torch.no_grad()
def validate_u8(net, lpnet, lq_u8, gt_u8, ratio_mode="gt", crop_border=0, bgr=True, tile=None, ratio_from="frame", overlap=0, batch=8,
                blend="average", ensemble=1, correct=None, sharpness=False, bracket=None, fusion=(1, 1, 1), ratio=None):
    """One validation step of the reference (image_restoration_model.py:578-586, :650-658, :746-748, :844-848) for a batch, on the device:
    uint8 low-quality and ground-truth frames [B,h,w,3] -> (uint8 result [B,h,w,3], PSNR list, SSIM list, ratio [B,1]).
    ratio_mode: "gt" feeds mean(gray(lq)) / mean(gray(gt)) as the validation does (gt_ratio; lpnet is not used and may be None),
    "lolblur" / "lolv1" feed LPNet's ratio as enhance_u8 does, "fixed" the caller's `ratio` [B,1] (neither the ground truth's nor LPNet's:
    what a chosen brightness scores).  The scores are calculate_psnr / calculate_ssim of the uint8 result
    (img1) against gt_u8, as the reference scores tensor2img's images (fdn_hip.metrics.calculate_psnr_ssim_u8).  Eager forward on the
    caller's stream.
    tile / ratio_from / overlap / batch / blend as in enhance_u8; ratio_from "tile" is the reference's val.grids validation.  With a tile
    the returned ratio is [B,T,1], one row per tile.  ensemble as in enhance_u8: the same ratio, the averaged result scored.
    correct: None, or "gt_mean" / "mean_var": two more values are returned, the PSNR list and the SSIM list of the result after that
    brightness correction towards gt_u8 (fdn_hip.correct.calculate_psnr_ssim_corrected_u8); the first four are what they are without.
    sharpness: True appends one more value after those, the list of fdn_hip.sharpness.sharpness_metrics(gt_u8, result): per frame the
    edge error, GMSD and the mean gradients with their ratio.
    bracket / fusion as in enhance_u8: the result scored is the fusion of the frame's renderings at the stops around the ratio fed
    without a bracket, which is the ratio returned."""
    from .ensemble import check_ensemble
    from .metrics import calculate_psnr_ssim_u8
    from .tiling import check_blend
    if correct is not None:
        from .correct import calculate_psnr_ssim_corrected_u8, check_mode
        check_mode(correct)

    def scored(out, ratio):
        psnr, ssim = calculate_psnr_ssim_u8(out, gt_u8, crop_border=crop_border, bgr=bgr)
        res = (out, psnr, ssim, ratio)
        if correct is not None:
            res += tuple(calculate_psnr_ssim_corrected_u8(gt_u8, out, correct, crop_border=crop_border, bgr=bgr))
        if sharpness:
            from .sharpness import sharpness_metrics
            res += (sharpness_metrics(gt_u8, out, bgr=bgr),)
        return res
    if ratio_mode not in ("gt", "lolblur", "lolv1", "fixed") or (ratio_mode == "fixed" and ratio is None):
        raise ValueError(f"ratio_mode {ratio_mode!r}" + (" needs ratio [B,1]" if ratio_mode == "fixed" else ""))
    check_blend(blend)
    check_ensemble(ensemble)
    if bracket is not None:
        from .fusion import check_bracket, check_exponents
        bracket, fusion = check_bracket(bracket), check_exponents(fusion)
    if ratio_mode not in ("gt", "fixed") and lpnet is None:
        raise FdnHipError(f"ratio_mode {ratio_mode!r} needs lpnet")
    if lq_u8.dim() == 3:
        lq_u8 = lq_u8.unsqueeze(0)
    if gt_u8.dim() == 3:
        gt_u8 = gt_u8.unsqueeze(0)
    if lq_u8.shape != gt_u8.shape:
        raise FdnHipError(f"Image shapes are different: {tuple(lq_u8.shape)}, {tuple(gt_u8.shape)}.")
    if ratio_mode == "fixed" and tuple(ratio.shape) != (lq_u8.shape[0], 1):
        raise FdnHipError(f"ratio_mode 'fixed' needs ratio [B,1] for B = {lq_u8.shape[0]}")
    if tile is not None and lq_u8.dim() == 4 and resolve_tile(tile, lq_u8.shape[1], lq_u8.shape[2]) is not None:
        done = [enhance_frame_tiled(net, lpnet, lq_u8[b], tile, bgr=bgr, ratio_mode=ratio_mode, ratio_from=ratio_from, gt_u8=gt_u8[b],
                                    ratio=None if ratio is None else ratio[b].reshape(-1, 1),
                                    overlap=overlap, batch=batch, blend=blend, ensemble=ensemble, bracket=bracket, fusion=fusion)
                for b in range(lq_u8.shape[0])]
        return scored(torch.stack([o for o, _ in done]), torch.stack([r for _, r in done]))
    x, h, w = preprocess(lq_u8, bgr=bgr)
    if ratio_mode == "gt":
        ratio = gt_ratio(x, preprocess(gt_u8, bgr=bgr)[0])
    elif ratio_mode == "fixed":
        ratio = ratio.to(device=x.device, dtype=torch.float32)
    elif ratio_mode == "lolblur":
        ratio = lpnet(x)
    else:
        ratio = lolv1_ratio(x, lpnet(x))
    ratio = ratio.contiguous()
    if bracket is not None:
        out = _bracket_u8(net, lq_u8, ratio, bracket, fusion, batch, ensemble, bgr)
    elif ensemble != 1:
        out = _ensemble_u8(net, lq_u8, ratio, ensemble, batch, h, w, bgr)
    else:
        out = postprocess(net(x, ratio_i=ratio, device=x.device)[0].contiguous(), h, w, bgr=bgr)
    return scored(out, ratio)


# ---------------------------------------------------------------------------------------------------------------------------------
# Video frames: Y'CbCr 4:2:0 as decoders hand it out (include/fdn_video.h)
# ---------------------------------------------------------------------------------------------------------------------------------
_PIX_FMTS = {"yuv420p": (0, 8), "nv12": (1, 8), "yuv420p10le": (0, 10)}       # ffmpeg's names -> (layout, bits)
_MATRICES = {"bt601": 0, "bt709": 1}
_CHROMA_LOCS = {"left": 0, "center": 1}


@dataclass(frozen=True)
class VideoFormat:
    """How the samples of a 4:2:0 frame are laid out and what they mean.  pix_fmt: yuv420p (planar 8 bit), nv12 (semi-planar 8 bit) or
    yuv420p10le (planar, 10 bits in little-endian 16-bit words); matrix: bt601 | bt709; full_range: codes 0 .. 2^bits - 1 instead of the
    limited 16 .. 235 / 240 (x 4 at 10 bit); chroma_loc: left (H.264 / HEVC default) | center (JPEG / MPEG-1)."""
    pix_fmt: str = "yuv420p"
    matrix: str = "bt709"
    full_range: bool = False
    chroma_loc: str = "left"

    def __post_init__(self):
        if self.pix_fmt not in _PIX_FMTS:
            raise ValueError(f"pix_fmt {self.pix_fmt!r}: one of {', '.join(_PIX_FMTS)}")
        if self.matrix not in _MATRICES:
            raise ValueError(f"matrix {self.matrix!r}: bt601 or bt709")
        if self.chroma_loc not in _CHROMA_LOCS:
            raise ValueError(f"chroma_loc {self.chroma_loc!r}: left or center")

    @property
    def layout(self):
        return _PIX_FMTS[self.pix_fmt][0]

    @property
    def bits(self):
        return _PIX_FMTS[self.pix_fmt][1]

    @property
    def dtype(self):
        """the sample type postprocess_yuv420 writes: uint8, or int16 for 10 bit (the codes 0 .. 1023 read the same as uint16)"""
        return torch.uint8 if self.bits == 8 else torch.int16

    @property
    def sample_bytes(self):
        return 1 if self.bits == 8 else 2

    def frame_samples(self, h, w):
        if h <= 0 or w <= 0 or h % 2 or w % 2:
            raise FdnHipError(f"a 4:2:0 frame needs even, positive sides, got {h}x{w}")
        return h * w * 3 // 2

    def _codes(self):
        return self.layout, self.bits, _MATRICES[self.matrix], int(bool(self.full_range)), _CHROMA_LOCS[self.chroma_loc]


def _yuv_frames(frames, h, w, fmt):
    """frames as preprocess_yuv420 takes them -> [B, frame_samples]; dtype and size are judged before where the tensor lives"""
    ok = (torch.uint8,) if fmt.bits == 8 else (torch.int16, torch.uint16)
    if not isinstance(frames, torch.Tensor) or frames.dtype not in ok:
        raise FdnHipError(f"{fmt.pix_fmt} frames must be {' or '.join(str(d) for d in ok)} tensors, got {getattr(frames, 'dtype', type(frames))}")
    if frames.dim() == 1:
        frames = frames.unsqueeze(0)
    n = fmt.frame_samples(h, w)
    if frames.dim() != 2 or frames.shape[1] != n or frames.shape[0] < 1:
        raise FdnHipError(f"expected {fmt.pix_fmt} frames [B, {n}] for {h}x{w}, got {tuple(frames.shape)}")
    return frames


def _yuv_ptr(t, what):
    if not t.is_cuda or not t.is_contiguous():
        raise FdnHipError(f"{what} must be a contiguous ROCm tensor")
    return ctypes.c_void_p(t.data_ptr())


def preprocess_yuv420(frames, h, w, fmt, pad=True):
    """4:2:0 frames [B, h*w*3/2] (uint8, or int16 / uint16 for 10 bit) on the GPU -> (fp32 [B,3,H,W] R'G'B' in [0,1], h, w): chroma
    interpolated to the luma grid, converted with fmt's matrix and range, clamped to the gamut, reflect-padded bottom / right to the x32
    grid like preprocess - or not at all with pad=False (H, W = h, w: the frame the tiled route cuts its tiles from)."""
    frames = _yuv_frames(frames, h, w, fmt)
    H, W = padded_size(h, w) if pad else (h, w)
    if H - h >= h or W - w >= w:
        raise FdnHipError(f"reflect padding {h}x{w} -> {H}x{W} needs pad < size (F.pad raises the same way)")
    src = _yuv_ptr(frames, "frames")
    out = torch.empty((frames.shape[0], 3, H, W), device=frames.device, dtype=torch.float32)
    check(lib().fdn_pre_yuv420(src, ctypes.c_void_p(out.data_ptr()), frames.shape[0], h, w, H, W, *fmt._codes(), stream()), "fdn_pre_yuv420")
    return out, h, w


def postprocess_yuv420(result, h, w, fmt):
    """fp32 [B,3,H,W] -> 4:2:0 frames [B, h*w*3/2] of fmt.dtype: crop, clamp(0,1), R'G'B' -> Y'CbCr, chroma downsampled from the cropped
    region, scaled to fmt's range, rounded half to even."""
    if not result.is_cuda or result.dtype != torch.float32 or not result.is_contiguous() or result.dim() != 4:
        raise FdnHipError("result must be a contiguous float32 ROCm tensor [B,3,H,W]")
    B, C, H, W = result.shape
    if C != 3 or h > H or w > W:
        raise FdnHipError(f"cannot crop {h}x{w} out of {tuple(result.shape)}")
    out = torch.empty((B, fmt.frame_samples(h, w)), device=result.device, dtype=fmt.dtype)
    check(lib().fdn_post_yuv420(ctypes.c_void_p(result.data_ptr()), _yuv_ptr(out, "out"), B, h, w, H, W, *fmt._codes(), stream()),
          "fdn_post_yuv420")
    return out


@torch.no_grad()
def enhance_yuv420(net, lpnet, frames, h, w, fmt, ratio_mode="lolblur", ratio=None, tile=None, ratio_from="frame", overlap=0, batch=8,
                   blend="average", temporal=None, denoise=None):
    """4:2:0 frames in -> 4:2:0 frames out, shaped and typed like the input, through LPNet -> FDN: enhance_u8 for video.  frames and fmt
    as preprocess_yuv420 takes them; every other keyword means what it means in enhance_u8.  Untiled, the batch goes through one forward;
    with a tile that resolve_tile turns into a crop, frame by frame: preprocess_yuv420(pad=False) -> tiling.split -> the ratio (from the
    reflect-padded frame, or per tile) -> tiling.run_tiles -> tiling.merge(blend) -> postprocess_yuv420.
    temporal: None, or the fdn_hip.temporal.RatioFilter of the stream these frames continue: what FDN would be fed per frame (frame_ratio:
    LPNet's prediction, or mean(gray) / LPNet for "lolv1") is filtered across the frames on the device, then fed as the "fixed" mode
    feeds a ratio; with a tile the frame's filtered ratio goes to every tile (ratio_from "frame" only).
    denoise: None, or the fdn_hip.mctf.TemporalDenoiser of the stream these frames continue: the fp32 frame - the forward's result, or the
    merged frame of the tiled route - goes through denoise.step before postprocess_yuv420 rounds it to samples."""
    from . import tiling
    if ratio_mode not in ("lolblur", "lolv1", "fixed"):
        raise ValueError(f"ratio_mode {ratio_mode!r}")
    tiling.check_blend(blend)
    if temporal is not None:
        if ratio_mode == "fixed":
            raise ValueError("temporal with ratio_mode 'fixed': a ratio the caller sets is not filtered")
        if ratio_from != "frame":
            raise ValueError(f"temporal with ratio_from {ratio_from!r}: the filter keeps one ratio per frame, not per tile")
        if not temporal.matches(h, w, fmt.bits):
            raise ValueError(f"temporal filter is for {temporal.h}x{temporal.w} {temporal.bits}-bit frames, these are {h}x{w} {fmt.bits}-bit")
        if lpnet is None:
            raise FdnHipError(f"ratio_mode {ratio_mode!r} needs lpnet")
    if denoise is not None and not denoise.matches(h, w, fmt.bits):
        raise ValueError(f"temporal denoiser is for {denoise.h}x{denoise.w} {denoise.bits}-bit frames, these are {h}x{w} {fmt.bits}-bit")
    frames = _yuv_frames(frames, h, w, fmt)
    B = frames.shape[0]
    crop = resolve_tile(tile, h, w)
    if crop is None:
        x = preprocess_yuv420(frames, h, w, fmt)[0]
        if temporal is not None:
            ratio_mode, ratio = "fixed", temporal.step(frames, frame_ratio(lpnet, x, ratio_mode).contiguous())
        res = _forward(net, lpnet, x, ratio_mode, ratio).contiguous()
        if denoise is not None:
            res = denoise.step(res)
        return postprocess_yuv420(res, h, w, fmt).view(frames.dtype)
    if ratio_mode == "fixed" and (ratio is None or ratio.shape[0] != B):
        raise FdnHipError(f"ratio_mode 'fixed' needs ratio [B,1] or [B,T,1] for B = {B}")
    ch, cw = tiling.effective_crop(h, w, *crop)
    out = []
    for b in range(B):
        frame = frames[b:b + 1]
        tiles, ij = tiling.split(preprocess_yuv420(frame, h, w, fmt, pad=False)[0], ch, cw, overlap)
        if temporal is not None:
            r = frame_ratio(lpnet, preprocess_yuv420(frame, h, w, fmt)[0], ratio_mode).contiguous()
            r = temporal.step(frame, r).expand(tiles.shape[0], 1).contiguous()
        else:
            r = _tile_ratio(lpnet, tiles, ratio_mode, ratio_from, None if ratio is None else ratio[b].reshape(-1, 1), batch,
                            lambda: preprocess_yuv420(frame, h, w, fmt)[0])
        res = tiling.merge(tiling.run_tiles(net, tiles, r, batch), ij, h, w, blend)
        if denoise is not None:
            res = denoise.step(res.contiguous())
        out.append(postprocess_yuv420(res, h, w, fmt))
    return torch.cat(out).view(frames.dtype)
