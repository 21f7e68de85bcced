"""Validation metrics on the GPU: the reference's basicsr/metrics/psnr_ssim.py `calculate_psnr` (:8-73) and `calculate_ssim`
(:243-328) with all their branches - the default 3-D Gaussian SSIM (`ssim3d=True`, :163-197), the 2-D one (`ssim3d=False`, `_ssim`
:84-116) and the Y-channel variants (`test_y_channel=True`: `to_y_channel` + `_ssim_cly` :199-240) - for (C,H,W) or (1,C,H,W) float32
ROCm tensors.  With `test_y_channel` the channels must be in B, G, R order and the range [0, 255], as the reference's callers pass
them (`tensor2img(..., rgb2bgr=True)`).  No CPU fallback.

`calculate_psnr_ssim_u8` scores batches of 8-bit images, what the reference's validation (image_restoration_model.py:746-748, :844-848)
and scripts/metrics/calculate_psnr_ssim.py do: the default branch in two launches over the uint8 batch (csrc/metrics_pair.hip).

The same package's no-reference metric, `calculate_niqe` (basicsr/metrics/niqe.py:67-205), is here too: the plane, the MSCN planes
and the per-block features on the GPU (csrc/niqe.hip), the 36-feature MVG fit on the host in float64 with the reference's own calls.

`calculate_lpips` is scripts/metrics/calculate_lpips.py's per-image step: LPIPS v0.1 (fdn_hip.lpips, csrc/lpips.hip) of 8-bit images."""
import ctypes
import math
import os

import numpy as np
import torch

from . import FdnHipError, check, lib, ptr, stream


def _prep(img1, img2, crop_border):
    if img1.shape != img2.shape:
        raise FdnHipError(f"Image shapes are different: {tuple(img1.shape)}, {tuple(img2.shape)}.")      # psnr_ssim.py:30
    out = []
    for t in (img1, img2):
        if t.dim() == 4:
            t = t.squeeze(0)
        if t.dim() != 3 or not t.is_cuda or t.dtype != torch.float32:
            raise FdnHipError("metrics take float32 ROCm tensors of shape (C,H,W) or (1,C,H,W)")
        if crop_border:
            t = t[:, crop_border:-crop_border, crop_border:-crop_border]
        out.append(t.contiguous())
    return out


def _sse_max(a, b):
    acc = torch.zeros(2, dtype=torch.float64, device=a.device)
    check(lib().fdn_sse_max(ptr(a), ptr(b), ctypes.c_long(a.numel()), ptr(acc), stream()), "fdn_sse_max")
    sse, mx = acc.tolist()
    return sse, mx


def to_y_channel(img_bgr):
    """(3,H,W) B,G,R in [0, 255] -> (1,H,W) Y in [16, 235] (metric_util.py:34-47)."""
    if img_bgr.shape[0] != 3:
        raise FdnHipError("to_y_channel needs a 3-channel (B, G, R) image")
    _, H, W = img_bgr.shape
    out = torch.empty((1, H, W), dtype=torch.float32, device=img_bgr.device)
    check(lib().fdn_y_channel(ptr(img_bgr), ptr(out), H, W, stream()), "fdn_y_channel")
    return out


def calculate_psnr(img1, img2, crop_border=0, test_y_channel=False):
    a, b = _prep(img1, img2, crop_border)
    if test_y_channel:                                                                                 # :55-57
        a, b = to_y_channel(a), to_y_channel(b)
    sse, mx = _sse_max(a, b)
    mse = sse / a.numel()
    if mse == 0:
        return float("inf")
    max_value = 1.0 if mx <= 1 else 255.0                                                              # :60
    return 20.0 * math.log10(max_value / math.sqrt(mse))


def _ssim2d(a, b, max_value, replicate_no_crop):
    C, H, W = a.shape
    ws = torch.empty(5 * a.numel(), dtype=torch.float64, device=a.device)
    acc = torch.zeros(1, dtype=torch.float64, device=a.device)
    check(lib().fdn_ssim2d(ptr(a), ptr(b), C, H, W, ctypes.c_float(max_value), int(replicate_no_crop), ptr(ws), ptr(acc), stream()),
          "fdn_ssim2d")
    count = C * H * W if replicate_no_crop else C * (H - 10) * (W - 10)
    return float(acc.item()) / count


def calculate_ssim(img1, img2, crop_border=0, test_y_channel=False, ssim3d=True):
    a, b = _prep(img1, img2, crop_border)
    if test_y_channel:                                                                                 # :275-278: Y plane, _ssim_cly
        return _ssim2d(to_y_channel(a), to_y_channel(b), 255.0, True)
    C, H, W = a.shape
    mx = float(a.max().item())
    max_value = 1.0 if mx <= 1 else 255.0                                                              # :286
    if not ssim3d:
        return _ssim2d(a, b, max_value, False)                                                         # _ssim, :84-116
    ws = torch.empty(10 * a.numel(), dtype=torch.float32, device=a.device)
    acc = torch.zeros(1, dtype=torch.float64, device=a.device)
    check(lib().fdn_ssim3d(ptr(a), ptr(b), C, H, W, ctypes.c_float(max_value), ptr(ws), ptr(acc), stream()), "fdn_ssim3d")
    return float(acc.item()) / a.numel()


# ---- paired validation on batches of 8-bit images (image_restoration_model.py:746-748, :844-848; scripts/metrics/calculate_psnr_ssim.py) --
PAIR_PARTS = 256                                          # FDN_PAIR_PARTS of include/fdn_hip.h: int64 partial pairs per image of fdn_pair_sse_u8


def ssim3d_taps():
    """cv2.getGaussianKernel(11, 1.5), float64 [11]: exp(-(i - 5)^2 / (2 sigma^2)) normalised (psnr_ssim.py:153-156)"""
    i = np.arange(11, dtype=np.float64) - 5.0
    k = np.exp(-(i * i) / (2.0 * 1.5 * 1.5))
    return k / k.sum()


def ssim3d_channel_matrix():
    """The channel pass of the 11 x 11 x 11 window over a 3-channel image with replicate padding (:158), float64 [c_out][c_in]: tap t of
    output channel c reads channel clamp(c + t - 5, 0, 2), so the pass is this 3 x 3 matrix of tap sums."""
    k, m = ssim3d_taps(), np.zeros((3, 3))
    for co in range(3):
        for t in range(11):
            m[co, min(max(co + t - 5, 0), 2)] += k[t]
    return m


def _u8_pair(img1, img2, crop_border, what="calculate_psnr_ssim_u8"):
    """-> (a, b, single): two contiguous uint8 [B][h][w][3] tensors on one ROCm device; `what` names the caller in the errors"""
    s1, s2 = tuple(getattr(img1, "shape", ())), tuple(getattr(img2, "shape", ()))
    if s1 != s2:
        raise FdnHipError(f"Image shapes are different: {s1}, {s2}.")                                # psnr_ssim.py:30
    out = []
    for img in (img1, img2):
        if isinstance(img, np.ndarray):
            img = torch.from_numpy(np.ascontiguousarray(img))
        if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8 or img.dim() not in (3, 4) or img.shape[-1] != 3:
            raise FdnHipError(f"{what} takes uint8 images (h,w,3) or (B,h,w,3), numpy arrays or tensors, got "
                              f"{getattr(img, 'dtype', type(img).__name__)} {tuple(getattr(img, 'shape', ()))}")
        out.append(img if img.dim() == 4 else img.unsqueeze(0))
    cb = int(crop_border)
    B, h, w, _ = out[0].shape
    if cb < 0:
        raise FdnHipError("crop_border must be >= 0")
    if B < 1 or h <= 2 * cb or w <= 2 * cb:
        raise FdnHipError(f"{what}: nothing is left of {B} image(s) of {h}x{w} with crop_border={cb}")
    devs = {t.device for t in out if t.is_cuda}
    if len(devs) > 1:
        raise FdnHipError(f"{what}: the two images are on different devices ({out[0].device}, {out[1].device})")
    dev = next(iter(devs), None)
    if dev is None:
        if not torch.cuda.is_available():
            raise FdnHipError(f"{what} needs a ROCm device; there is no CPU fallback")
        dev = torch.device("cuda", torch.cuda.current_device())
    return out[0].to(dev).contiguous(), out[1].to(dev).contiguous(), len(s1) == 3


def _psnr_from_sse(sse, mx, n):
    mse = sse / n                                                                                      # :59 (integers: exact)
    if mse == 0:
        return float("inf")                                                                            # :60-61
    return 20.0 * math.log10((1.0 if mx <= 1 else 255.0) / math.sqrt(mse))                              # :62-63


def calculate_psnr_ssim_u8(img1, img2, crop_border=0, test_y_channel=False, ssim3d=True, bgr=True):
    """calculate_psnr and calculate_ssim (psnr_ssim.py:8-70, :243-329) of 8-bit image pairs, as the reference's validation and its
    scripts/metrics/calculate_psnr_ssim.py score them: (h,w,3) or (B,h,w,3) uint8 numpy arrays or tensors (host data is moved to the
    current ROCm device).  img1 decides the peak value (img1.max() <= 1 -> 1, else 255).  -> (psnr, ssim): two floats for one pair, two
    lists of B floats for a batch.  The default branch (RGB PSNR, 3-D SSIM) is two kernels over the whole batch and one device-to-host
    copy; the scores are bit-identical across calls and do not depend on the rest of the batch.  test_y_channel=True and ssim3d=False
    go image by image through the float32 entry points (calculate_psnr / calculate_ssim above).  bgr says whether the channels are
    B, G, R (cv2.imread, tensor2img) or R, G, B; only the Y channel depends on it (the 3-D window is symmetric along the channel axis)."""
    a, b, single = _u8_pair(img1, img2, crop_border)
    cb = int(crop_border)
    B, h, w, _ = a.shape
    if test_y_channel or not ssim3d:
        psnr, ssim = [], []
        for i in range(B):
            x, y = (t[i].permute(2, 0, 1).to(torch.float32) for t in (a, b))                           # (3,h,w) planes, values 0..255
            if test_y_channel and not bgr:
                x, y = x.flip(0), y.flip(0)
            psnr.append(calculate_psnr(x, y, cb, test_y_channel))
            ssim.append(calculate_ssim(x, y, cb, test_y_channel, ssim3d))
    else:
        l = lib()
        nws = int(l.fdn_pair_ssim3d_ws(B, h, w, cb))
        stats = torch.empty((B, PAIR_PARTS, 2), dtype=torch.int64, device=a.device)
        ws = torch.empty(max(nws, 1), dtype=torch.float64, device=a.device)
        out = torch.empty((B, 3), dtype=torch.float64, device=a.device)
        taps, mix = ssim3d_taps(), np.ascontiguousarray(ssim3d_channel_matrix())
        with torch.cuda.device(a.device):
            s = stream()
            check(l.fdn_pair_sse_u8(ptr(a), ptr(b), B, h, w, cb, ptr(stats), s), "fdn_pair_sse_u8")
            check(l.fdn_pair_ssim3d_u8(ptr(a), ptr(b), B, h, w, cb, ptr(stats), taps.ctypes.data_as(ctypes.c_void_p),
                                       mix.ctypes.data_as(ctypes.c_void_p), ptr(ws), ptr(out), s), "fdn_pair_ssim3d_u8")
        res = out.cpu().tolist()                                                                       # the one copy: [B][sse, max, ssim]
        n = 3 * (h - 2 * cb) * (w - 2 * cb)
        psnr = [_psnr_from_sse(int(r[0]), r[1], n) for r in res]
        ssim = [r[2] for r in res]
    return (psnr[0], ssim[0]) if single else (psnr, ssim)


# ---- NIQE (basicsr/metrics/niqe.py) ------------------------------------------------------------------------------------------------------
NIQE_BLOCK = 96                                                                                       # block_size_h / _w (:70-71)
_LUMA_MODE = {"y": 0, "gray": 1}
_niqe_tables_dev = {}       # device -> float64 tensor [4][9801] of fdn_niqe_features: built once per device, as ops._fdsa_scratch is


def niqe_tables():
    """The AGGD search tables of estimate_aggd_param (:21-37), float64 [4][9801] on the host: gam = np.arange(0.2, 10.001, 0.001),
    r_gam = gamma(2/a)^2 / (gamma(1/a) gamma(3/a)) with the reference's 1/a * 2, 1/a * 3, then sqrt(gamma(1/a) / gamma(3/a)) and
    gamma(2/a) / gamma(1/a) as :35-36 and :61 form them.  math.gamma, so that the product does not depend on scipy."""
    gam = np.arange(0.2, 10.001, 0.001)
    rec = np.reciprocal(gam)
    g = math.gamma
    r_gam = np.array([g(r * 2) * g(r * 2) / (g(r) * g(r * 3)) for r in rec.tolist()])
    beta = np.array([math.sqrt(g(1 / a) / g(3 / a)) for a in gam.tolist()])
    mean = np.array([g(2 / a) / g(1 / a) for a in gam.tolist()])
    return np.stack([gam, r_gam, beta, mean])


def _niqe_tables_on(device):
    t = _niqe_tables_dev.get(str(device))
    if t is None:
        t = _niqe_tables_dev[str(device)] = torch.from_numpy(niqe_tables()).to(device)
    return t


def niqe_params(params=None):
    """(mu_pris_param [1,36], cov_pris_param [36,36], gaussian_window [7,7]), float64.  params: a path to niqe_pris_params.npz, a
    mapping with those three keys, or None: basicsr/metrics/niqe_pris_params.npz of the reference checkout behind this package, found
    along `basicsr.__path__`."""
    if params is None:
        import basicsr
        for d in basicsr.__path__:
            f = os.path.join(d, "metrics", "niqe_pris_params.npz")
            if os.path.isfile(f):
                params = f
                break
        else:
            raise FdnHipError("calculate_niqe: no basicsr/metrics/niqe_pris_params.npz along basicsr.__path__ (put the reference checkout "
                              "on sys.path after this package, or pass params=<path to niqe_pris_params.npz or a mapping>)")
    if isinstance(params, (str, os.PathLike)):
        with np.load(params) as z:
            params = {k: z[k] for k in z.files}
    try:
        mu = np.asarray(params["mu_pris_param"], dtype=np.float64).reshape(1, 36)
        cov = np.asarray(params["cov_pris_param"], dtype=np.float64).reshape(36, 36)
        win = np.asarray(params["gaussian_window"], dtype=np.float64)
    except (KeyError, ValueError) as e:
        raise FdnHipError(f"calculate_niqe: params need mu_pris_param [1,36], cov_pris_param [36,36] and gaussian_window [7,7] ({e})")
    if win.shape != (7, 7):
        raise FdnHipError(f"calculate_niqe: gaussian_window must be 7x7, got {win.shape}")
    return mu, cov, win


def niqe_features(img, crop_border=0, input_order="CHW", convert_to="y", window=None):
    """The GPU part of calculate_niqe for (H,W) ('HW'), (C,H,W) or (B,C,H,W) float32 ROCm tensors in [0, 255], B, G, R order.
    Returns a dict of device tensors: "plane" [B][H][W] (the scored plane, cut to whole 96x96 blocks), "mscn1" [B][H][W],
    "mscn2" [B][H/2][W/2] and "feats" [2][B][nblocks][18] float64 (scale 1, scale 2; blocks idx_w outer, idx_h inner)."""
    if not isinstance(img, torch.Tensor) or not img.is_cuda or img.dtype != torch.float32:
        raise FdnHipError("calculate_niqe takes float32 ROCm tensors")
    if input_order == "HW":
        if img.dim() != 2:
            raise FdnHipError(f"input_order='HW' needs an (H, W) tensor, got {tuple(img.shape)}")
        x, mode = img.reshape(1, 1, *img.shape), 2
    elif input_order == "CHW":
        if img.dim() not in (3, 4):
            raise FdnHipError(f"input_order='CHW' needs a (C,H,W) or (B,C,H,W) tensor, got {tuple(img.shape)}")
        x = img if img.dim() == 4 else img.unsqueeze(0)
        if convert_to not in _LUMA_MODE:
            raise FdnHipError(f"convert_to must be 'y' or 'gray', got {convert_to!r}")
        mode = _LUMA_MODE[convert_to]
        if x.shape[1] != 3 and not (x.shape[1] == 1 and mode == 0):
            raise FdnHipError(f"convert_to={convert_to!r} needs 3 channels (B, G, R){' or 1' if mode == 0 else ''}, got {x.shape[1]}")
    else:
        raise FdnHipError(f"input_order must be 'HW' or 'CHW', got {input_order!r}")
    B, C, Hs, Ws = x.shape
    cb = int(crop_border)
    if cb < 0:
        raise FdnHipError("crop_border must be >= 0")
    nbh, nbw = (Hs - 2 * cb) // NIQE_BLOCK, (Ws - 2 * cb) // NIQE_BLOCK
    if nbh < 1 or nbw < 1:
        raise FdnHipError(f"calculate_niqe: {Hs}x{Ws} with crop_border={cb} holds no whole {NIQE_BLOCK}x{NIQE_BLOCK} block")
    if window is None:
        window = niqe_params()[2]
    win = np.ascontiguousarray(window, dtype=np.float64).reshape(49)
    x = x.contiguous()
    H, W = nbh * NIQE_BLOCK, nbw * NIQE_BLOCK
    dev = x.device
    plane = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    mscn1 = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    mscn2 = torch.empty((B, H // 2, W // 2), dtype=torch.float32, device=dev)
    feats = torch.empty((2, B, nbh * nbw, 18), dtype=torch.float64, device=dev)
    tables = _niqe_tables_on(dev)
    l, s = lib(), stream()
    wp = win.ctypes.data_as(ctypes.c_void_p)
    check(l.fdn_niqe_luma(ptr(x), ptr(plane), B, C, Hs, Ws, cb, cb, H, W, mode, s), "fdn_niqe_luma")
    check(l.fdn_niqe_mscn(ptr(plane), ptr(mscn1), B, H, W, 0, wp, s), "fdn_niqe_mscn")
    check(l.fdn_niqe_mscn(ptr(plane), ptr(mscn2), B, H // 2, W // 2, 1, wp, s), "fdn_niqe_mscn")
    ntab = tables.shape[1]
    check(l.fdn_niqe_features(ptr(mscn1), ptr(feats[0]), B, H, W, NIQE_BLOCK, ptr(tables), ntab, s), "fdn_niqe_features")
    check(l.fdn_niqe_features(ptr(mscn2), ptr(feats[1]), B, H // 2, W // 2, NIQE_BLOCK // 2, ptr(tables), ntab, s), "fdn_niqe_features")
    return {"plane": plane, "mscn1": mscn1, "mscn2": mscn2, "feats": feats}


def niqe_score(distparam, mu_pris_param, cov_pris_param):
    """The MVG fit of niqe() (:141-153) on the host in float64, with the reference's calls, for distparam [nblocks][36].  A row with a
    NaN drops out of the covariance but its other entries stay in the mean, as np.nanmean / the complete-row np.cov there do."""
    complete = distparam[~np.isnan(distparam).any(axis=1)]
    if complete.shape[0] < 2:
        raise FdnHipError(f"calculate_niqe: {complete.shape[0]} of {distparam.shape[0]} blocks have complete features (a flat image?); "
                          "the covariance needs at least 2")
    mu_distparam = np.nanmean(distparam, axis=0)
    cov_distparam = np.cov(complete, rowvar=False)
    invcov_param = np.linalg.pinv((cov_pris_param + cov_distparam) / 2)
    quality = np.matmul(np.matmul((mu_pris_param - mu_distparam), invcov_param), np.transpose((mu_pris_param - mu_distparam)))
    q = float(np.sqrt(quality).item())
    if not math.isfinite(q):
        raise FdnHipError(f"calculate_niqe: the score is not finite ({q})")
    return q


def calculate_niqe(img, crop_border=0, input_order="CHW", convert_to="y", params=None):
    """NIQE of calculate_niqe (basicsr/metrics/niqe.py:158-205) for float32 ROCm tensors in [0, 255], channels B, G, R.
    (H,W) with input_order='HW', (C,H,W) or (1,C,H,W) -> a float; (B,C,H,W) with B > 1 -> a list of B floats (one launch per kernel
    for the batch).  params: see niqe_params; convert_to: 'y' (Y of BT.601) or 'gray' (cv2.cvtColor BGR2GRAY)."""
    mu, cov, win = niqe_params(params)
    r = niqe_features(img, crop_border, input_order, convert_to, window=win)
    f = r["feats"].cpu().numpy()                                                                      # [2][B][nblocks][18]
    scores = [niqe_score(np.concatenate([f[0, b], f[1, b]], axis=1), mu, cov) for b in range(f.shape[1])]
    return scores if (img.dim() == 4 and img.shape[0] > 1) else scores[0]


# ---- LPIPS (scripts/metrics/calculate_lpips.py: lpips.LPIPS(net='vgg'), version 0.1) --------------------------------------------------------
_lpips_models = {}          # (net, weights path, lin path, device) -> (the files' (mtime, size), LPIPS): the weights are loaded once per file version and device


def _file_stamp(path):
    if path is None:
        return None
    st = os.stat(path)
    return st.st_mtime_ns, st.st_size


def lpips_model(net="vgg", weights=None, lin_weights=None, device=None):
    """fdn_hip.lpips.LPIPS for these weights; built once per (net, files, device) when the weights are given as paths, and again when
    a file has been rewritten in place (its modification time or size differs; the model of the old contents is dropped)"""
    from .lpips import LPIPS
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    paths = all(w is None or isinstance(w, (str, os.PathLike)) for w in (weights, lin_weights))
    if not paths:
        return LPIPS(net, weights, lin_weights, dev)
    key = (net, None if weights is None else os.path.abspath(weights), None if lin_weights is None else os.path.abspath(lin_weights), str(dev))
    stamp = (_file_stamp(key[1]), _file_stamp(key[2]))
    hit = _lpips_models.get(key)
    if hit is None or hit[0] != stamp:
        hit = _lpips_models[key] = (stamp, LPIPS(net, weights, lin_weights, dev))
    return hit[1]


def _u8_images(img, dev):
    if isinstance(img, np.ndarray):
        img = torch.from_numpy(np.ascontiguousarray(img))
    if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8 or img.dim() not in (3, 4) or img.shape[-1] != 3:
        raise FdnHipError("calculate_lpips takes uint8 images (H,W,3) or (B,H,W,3), numpy arrays or tensors, got "
                          f"{getattr(img, 'dtype', type(img).__name__)} {tuple(getattr(img, 'shape', ()))}")
    return (img if img.dim() == 4 else img.unsqueeze(0)).to(dev).contiguous()


def calculate_lpips(img1, img2, net="vgg", model=None, weights=None, lin_weights=None, bgr=True, device=None, per_layer=False):
    """LPIPS v0.1 of calculate_lpips.py (:44-54) for 8-bit images: (H,W,3) or (B,H,W,3) uint8 numpy arrays or tensors, channels B, G, R
    as cv2.imread gives them (bgr=False: R, G, B as PIL gives them).  img1 is lpips' in0 (the restored image in the reference script),
    img2 in1 (the ground truth); the metric is symmetric.  model: an fdn_hip.lpips.LPIPS, else one is built (once per file) from net,
    weights and lin_weights.  -> a float for one pair, a list of B floats for a batch (one backbone pass for all 2B images);
    per_layer=True gives the five heads' terms instead ([5] / [B][5] lists)."""
    if tuple(img1.shape) != tuple(img2.shape):
        raise FdnHipError(f"Image shapes are different: {tuple(img1.shape)}, {tuple(img2.shape)}.")      # as psnr_ssim.py:30
    if model is None:
        model = lpips_model(net, weights, lin_weights, device)
    a, b = _u8_images(img1, model.device), _u8_images(img2, model.device)
    d = model.from_u8(a, b, bgr=bgr, per_layer=per_layer).cpu().tolist()
    return d if len(img1.shape) == 4 and img1.shape[0] > 1 else d[0]
