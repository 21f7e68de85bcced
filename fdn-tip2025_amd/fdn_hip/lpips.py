"""LPIPS v0.1 on the GPU (Zhang et al. 2018): the `lpips` package's LPIPS(net='vgg' | 'alex', version='0.1') in eval mode, which the
reference's scripts/metrics/calculate_lpips.py runs with net='vgg' (and pyiqa's `lpips` metric, with net='alex').

    d(in0, in1) = sum_l mean_{h,w} sum_c w_{l,c} (f0_{l,c} / (|f0_l| + 1e-10) - f1_{l,c} / (|f1_l| + 1e-10))^2

with f_l the backbone's features at five taps after its ReLUs, for inputs passed through the scaling layer.  The backbone convs are
fdn_conv2d with FDN_ACT_RELU (the 3x3 ones on the split-bf16 matrix-core kernel), the pools fdn_maxpool2d, the scaling layer
fdn_lpips_prep_*, the five heads fdn_lpips_layer (csrc/lpips.hip).  No CPU fallback.

The weights are the user's (none ship with this package).  Accepted, as files (torch.load(weights_only=True)) or as mappings:
  (a) an lpips.LPIPS state_dict: net.sliceK.<idx>.weight|bias (torchvision's `features` indices), linK.model.1.weight and / or
      lins.K.model.1.weight (equal where both are given), optionally scaling_layer.shift|scale (checked against the constants);
  (b) a torchvision vgg16 / alexnet state_dict (features.<idx>.weight|bias; classifier.* is ignored) as `weights`, together with the
      lpips linear heads weights/v0.1/{vgg,alex}.pth (linK.model.1.weight, shape [1,C,1,1]) as `lin_weights`.
A missing key, an unexpected key or a wrong shape raises FdnHipError naming the key.  pyiqa's combined LPIPS files are expected to have
layout (a); that is untested."""
import os
from collections.abc import Mapping

import torch

from . import ACT_RELU, FdnHipError, check, lib, ops, ptr, stream

SHIFT = (-.030, -.088, -.188)            # ScalingLayer of lpips (float32 on the device, as torch.Tensor of these)
SCALE = (.458, .448, .450)
LPIPS_PARTS = 1024                       # FDN_LPIPS_PARTS of include/fdn_hip.h: workspace doubles per pair of fdn_lpips_layer

# torchvision `features` of each backbone, up to the fifth tap: ("conv", index, Cin, Cout, k, stride, pad) (+ ReLU), ("pool", k, s),
# ("tap",).  lpips' slice K (1-based) holds the convs after K - 1 taps, with their torchvision indices as module names.
ARCH = {
    "vgg": [("conv", 0, 3, 64, 3, 1, 1), ("conv", 2, 64, 64, 3, 1, 1), ("tap",), ("pool", 2, 2),
            ("conv", 5, 64, 128, 3, 1, 1), ("conv", 7, 128, 128, 3, 1, 1), ("tap",), ("pool", 2, 2),
            ("conv", 10, 128, 256, 3, 1, 1), ("conv", 12, 256, 256, 3, 1, 1), ("conv", 14, 256, 256, 3, 1, 1), ("tap",), ("pool", 2, 2),
            ("conv", 17, 256, 512, 3, 1, 1), ("conv", 19, 512, 512, 3, 1, 1), ("conv", 21, 512, 512, 3, 1, 1), ("tap",), ("pool", 2, 2),
            ("conv", 24, 512, 512, 3, 1, 1), ("conv", 26, 512, 512, 3, 1, 1), ("conv", 28, 512, 512, 3, 1, 1), ("tap",)],
    "alex": [("conv", 0, 3, 64, 11, 4, 2), ("tap",), ("pool", 3, 2),
             ("conv", 3, 64, 192, 5, 1, 2), ("tap",), ("pool", 3, 2),
             ("conv", 6, 192, 384, 3, 1, 1), ("tap",),
             ("conv", 8, 384, 256, 3, 1, 1), ("tap",),
             ("conv", 10, 256, 256, 3, 1, 1), ("tap",)],
}


def convs(net):
    """[(slice K, torchvision index, Cin, Cout, k, stride, pad)] of the backbone, in order"""
    if net not in ARCH:
        raise FdnHipError(f"LPIPS: net must be 'vgg' or 'alex', got {net!r}")
    out, taps = [], 0
    for op in ARCH[net]:
        if op[0] == "tap":
            taps += 1
        elif op[0] == "conv":
            out.append((taps + 1,) + op[1:])
    return out


def tap_channels(net):
    """channels of the five taps"""
    ch, c = [], 0
    for op in ARCH[net]:
        if op[0] == "conv":
            c = op[3]
        elif op[0] == "tap":
            ch.append(c)
    return ch


def tap_sizes(net, H, W):
    """(h, w) of the five taps for an H x W input; FdnHipError when a conv or pool of the backbone has nothing left to cover"""
    h, w = H, W
    out = []
    for op in ARCH[net]:
        if op[0] == "conv":
            _, _, _, _, k, s, p = op
            h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        elif op[0] == "pool":
            _, k, s = op
            if h < k or w < k:
                h = w = 0
            else:
                h, w = (h - k) // s + 1, (w - k) // s + 1
        else:
            out.append((h, w))
        if h < 1 or w < 1:
            raise FdnHipError(f"LPIPS({net}): {H}x{W} is too small, the backbone has nothing left before its tap {len(out) + 1}")
    return out


def _load(src, what):
    if isinstance(src, Mapping):
        return dict(src)
    if isinstance(src, (str, os.PathLike)):
        sd = torch.load(src, map_location="cpu", weights_only=True)
        if not isinstance(sd, Mapping):
            raise FdnHipError(f"LPIPS {what} {os.fspath(src)!r}: not a state_dict")
        return dict(sd)
    raise FdnHipError(f"LPIPS {what}: a path or a state_dict mapping, got {type(src).__name__}")


def _tensor(sd, key, shape):
    if key not in sd:
        raise FdnHipError(f"LPIPS weights: missing key {key!r}")
    t = sd[key]
    if not torch.is_tensor(t) or not t.is_floating_point():
        raise FdnHipError(f"LPIPS weights: {key!r} is not a floating-point tensor")
    if tuple(t.shape) != tuple(shape):
        raise FdnHipError(f"LPIPS weights: {key!r} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t.detach().to("cpu", torch.float32).contiguous()


def _lins(sd, net, what):
    """the five heads from linK.model.1.weight and / or lins.K.model.1.weight -> ([C] tensors, the keys used)"""
    out, used = [], set()
    for k, C in enumerate(tap_channels(net)):
        names = [n for n in (f"lin{k}.model.1.weight", f"lins.{k}.model.1.weight") if n in sd]
        if not names:
            raise FdnHipError(f"LPIPS {what}: missing key 'lin{k}.model.1.weight' (or 'lins.{k}.model.1.weight')")
        ts = [_tensor(sd, n, (1, C, 1, 1)) for n in names]
        if len(ts) == 2 and not torch.equal(ts[0], ts[1]):
            raise FdnHipError(f"LPIPS {what}: {names[0]!r} and {names[1]!r} differ")
        out.append(ts[0].reshape(C))
        used.update(names)
    return out, used


def load_weights(net, weights, lin_weights=None):
    """-> {"convs": [(weight [Cout][Cin][k][k], bias [Cout])], "lins": [[C]] * 5}, float32 contiguous CPU tensors, from layout (a)
    (an lpips.LPIPS state_dict; `lin_weights` then only if it lacks the heads) or (b) (a torchvision state_dict + `lin_weights`)."""
    spec = convs(net)
    sd = _load(weights, "weights")
    if any(k.startswith("features.") for k in sd):                                                   # (b) torchvision
        names = [(f"features.{i}.weight", f"features.{i}.bias") for _, i, *_ in spec]
        extra = [k for k in sd if not k.startswith("classifier.")]
        if lin_weights is None:
            raise FdnHipError(f"LPIPS({net}): a torchvision backbone needs lin_weights (the lpips weights/v0.1/{net}.pth)")
        lsd = _load(lin_weights, "lin_weights")
        lins, lused = _lins(lsd, net, "lin_weights")
        lextra = [k for k in lsd if k not in lused]
    elif any(k.startswith("net.") for k in sd):                                                      # (a) lpips.LPIPS
        names = [(f"net.slice{s}.{i}.weight", f"net.slice{s}.{i}.bias") for s, i, *_ in spec]
        has_lin = any(k.startswith(("lin", "lins.")) for k in sd)
        if lin_weights is not None and has_lin:
            raise FdnHipError("LPIPS: the weights hold linear heads and lin_weights were given too")
        lsd = _load(lin_weights, "lin_weights") if lin_weights is not None else sd
        lins, lused = _lins(lsd, net, "lin_weights" if lin_weights is not None else "weights")
        lextra = [k for k in lsd if k not in lused] if lin_weights is not None else []
        for key, const in (("scaling_layer.shift", SHIFT), ("scaling_layer.scale", SCALE)):
            if key in sd:
                t = sd[key]
                want = torch.tensor(const, dtype=torch.float32)
                if not torch.is_tensor(t) or t.numel() != 3 or not torch.equal(t.detach().cpu().reshape(3).to(torch.float32), want):
                    raise FdnHipError(f"LPIPS weights: {key!r} is {t if not torch.is_tensor(t) else t.reshape(-1).tolist()}, "
                                      f"LPIPS v0.1 has {list(const)}")
        extra = [k for k in sd if k not in lused and k not in ("scaling_layer.shift", "scaling_layer.scale")]
    else:
        raise FdnHipError("LPIPS weights: neither an lpips.LPIPS state_dict (net.sliceK.*) nor a torchvision one (features.*)")
    packed = []
    for (wk, bk), (_, _, cin, cout, k, _, _) in zip(names, spec):
        packed.append((_tensor(sd, wk, (cout, cin, k, k)), _tensor(sd, bk, (cout,))))
    want = {n for pair in names for n in pair}
    extra = [k for k in extra if k not in want] + lextra
    if extra:
        raise FdnHipError(f"LPIPS({net}) weights: unexpected key {sorted(extra)[0]!r}" + (f" (and {len(extra) - 1} more)" if len(extra) > 1 else ""))
    return {"convs": packed, "lins": lins}


def prep_u8(img, bgr=True):
    """uint8 [B][H][W][3] ROCm tensor -> the scaling layer's output float32 [B][3][H][W] (R, G, B), calculate_lpips.py's op order"""
    if not img.is_cuda or img.dtype != torch.uint8 or img.dim() != 4 or img.shape[3] != 3:
        raise FdnHipError(f"LPIPS: 8-bit images are uint8 ROCm tensors [B,H,W,3], got {img.dtype} {tuple(img.shape)} on {img.device}")
    img = img.contiguous()
    B, H, W, _ = img.shape
    out = torch.empty((B, 3, H, W), dtype=torch.float32, device=img.device)
    check(lib().fdn_lpips_prep_u8(ptr(img), ptr(out), B, H, W, int(bool(bgr)), stream()), "fdn_lpips_prep_u8")
    return out


def prep_f32(x, normalize=False, out=None):
    """float32 [B][3][H][W] in [-1, 1] (normalize=True: in [0, 1], taken through 2 x - 1) -> the scaling layer's output"""
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
        raise FdnHipError(f"LPIPS: inputs are float32 ROCm tensors [B,3,H,W], got {x.dtype} {tuple(x.shape)} on {x.device}")
    x = x.contiguous()
    B, _, H, W = x.shape
    if out is None:
        out = torch.empty_like(x)
    check(lib().fdn_lpips_prep_f32(ptr(x), ptr(out), B, H, W, int(bool(normalize)), stream()), "fdn_lpips_prep_f32")
    return out


def layer(f, w, out=None, accumulate=False):
    """one head: f [2B][C][H][W] (in0 images, then in1), w [C] -> out [B] float64 (added to `out` with accumulate=True)"""
    N, C, H, W = f.shape
    if N % 2 or not f.is_contiguous() or w.numel() != C:
        raise FdnHipError(f"fdn_lpips_layer: features [2B,C,H,W] contiguous and w [C], got {tuple(f.shape)} and {tuple(w.shape)}")
    B = N // 2
    if out is None:
        out = torch.zeros(B, dtype=torch.float64, device=f.device)
    ws = torch.empty(B * LPIPS_PARTS, dtype=torch.float64, device=f.device)
    check(lib().fdn_lpips_layer(ops._flat(f, "f"), ops._flat(w, "w"), ptr(out), B, C, H, W, int(bool(accumulate)), ptr(ws), stream()),
          "fdn_lpips_layer")
    return out


class LPIPS:
    """LPIPS v0.1 with the backbone `net` ('vgg' or 'alex').  The weights are loaded once (see the module's docstring for the layouts)
    and kept on `device` (default: the current ROCm device).  model(in0, in1) -> float64 [B] on the device, in0 / in1 float32
    [B,3,H,W] in [-1, 1] (normalize=True: in [0, 1]); per_layer=True -> [B,5], the five heads' terms."""

    def __init__(self, net="vgg", weights=None, lin_weights=None, device=None):
        if weights is None:
            raise FdnHipError("LPIPS: weights are needed (an lpips.LPIPS state_dict, or a torchvision one with lin_weights); none ship here")
        packed = load_weights(net, weights, lin_weights)
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if dev.type != "cuda":
            raise FdnHipError(f"LPIPS runs on a ROCm device, got {dev}; there is no CPU fallback")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.net, self.device = net, dev
        self.convs = [(w.to(dev), b.to(dev)) for w, b in packed["convs"]]
        self.lins = [l.to(dev) for l in packed["lins"]]

    def features(self, x):
        """the five taps of the backbone for x [N,3,H,W] (the scaling layer's output)"""
        taps, ci = [], 0
        for op in ARCH[self.net]:
            if op[0] == "conv":
                w, b = self.convs[ci]
                ci += 1
                x = ops.conv2d(x, w, b, stride=op[5], pad=op[6], act=ACT_RELU)
            elif op[0] == "pool":
                x = ops.maxpool2d(x, op[1], op[2])
            else:
                taps.append(x)
        return taps

    def _check(self, in0, in1):
        for t in (in0, in1):
            if not torch.is_tensor(t) or t.device != self.device or t.dim() != 4 or t.shape[1] != 3:
                raise FdnHipError(f"LPIPS: inputs are [B,3,H,W] tensors on {self.device}, got "
                                  f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}" + (f" on {t.device}" if torch.is_tensor(t) else ""))
        if in0.shape != in1.shape:
            raise FdnHipError(f"LPIPS: in0 and in1 differ in shape: {tuple(in0.shape)}, {tuple(in1.shape)}")
        tap_sizes(self.net, in0.shape[2], in0.shape[3])

    def _score(self, x, per_layer):
        B = x.shape[0] // 2
        taps = self.features(x)
        out = torch.empty((5, B) if per_layer else (B,), dtype=torch.float64, device=self.device)
        for l, (f, w) in enumerate(zip(taps, self.lins)):
            if per_layer:
                layer(f, w, out[l], accumulate=False)
            else:
                layer(f, w, out, accumulate=l > 0)
        return out.t().contiguous() if per_layer else out

    def __call__(self, in0, in1, normalize=False, per_layer=False):
        self._check(in0, in1)
        B, _, H, W = in0.shape
        with torch.cuda.device(self.device):
            x = torch.empty((2 * B, 3, H, W), dtype=torch.float32, device=self.device)
            prep_f32(in0, normalize, out=x[:B])
            prep_f32(in1, normalize, out=x[B:])
            return self._score(x, per_layer)

    def from_u8(self, img0, img1, bgr=True, per_layer=False):
        """the same for 8-bit images: uint8 [B,H,W,3] tensors on the device (bgr=True: B, G, R as cv2.imread gives), scored as
        calculate_lpips.py scores them (/ 255, normalize to [-1, 1])"""
        if img0.shape != img1.shape:
            raise FdnHipError(f"LPIPS: image shapes are different: {tuple(img0.shape)}, {tuple(img1.shape)}")
        if img0.device != self.device or img1.device != self.device:
            raise FdnHipError(f"LPIPS: images must be on {self.device}")
        if img0.dim() == 4:
            tap_sizes(self.net, img0.shape[1], img0.shape[2])
        with torch.cuda.device(self.device):
            x = torch.cat([prep_u8(img0, bgr), prep_u8(img1, bgr)])
            return self._score(x, per_layer)
