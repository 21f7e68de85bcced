"""Golden values for the paired 8-bit metrics (fdn_hip.metrics.calculate_psnr_ssim_u8): the reference's own calculate_psnr and
calculate_ssim (ssim3d=True), lifted by AST exactly as make_golden_metrics.py lifts them, run on uint8 HWC arrays
(input_order='HWC') - what its validation hands them after tensor2img.  Stored: the uint8 inputs, crop_border and the reference's
values.  The inputs are textured and not too bright: where the local variance is small beside x^2, E[x^2] - mu^2 cancels in float32 and
the reference's own value is rounding-limited (1e-4 on a smooth image around level 160 with noise of sigma 5).  An input is admitted
only if the reference's value lies within REF_ERR_MAX of the same formula in float64; that distance is stored with the case.
Run:  python tests/golden/make_golden_paired.py"""
import json
import os

import numpy as np
import torch

from make_golden_metrics import HERE, reference_functions


def smooth(rng, h, w, level, amp):
    """a smooth textured image: a few low-frequency waves per channel around `level`"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.empty((h, w, 3))
    for c in range(3):
        f = rng.uniform(0.02, 0.12, size=(3, 2))
        p = rng.uniform(0, 2 * np.pi, size=3)
        img[..., c] = level + amp * sum(np.sin(f[k, 0] * yy + f[k, 1] * xx + p[k]) for k in range(3)) / 3.0
    return img


def u8(a):
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def pairs():
    """name -> (img1, img2, crop_border); img1 [h][w][3] or, for the batch, [5][h][w][3]"""
    rng = np.random.default_rng(20)
    out = {}
    x = rng.integers(0, 256, (70, 90, 3))
    out["noise"] = (u8(x), u8(x + rng.integers(-30, 31, x.shape)), 0)
    s = smooth(rng, 96, 160, 110.0, 70.0)
    a, b = u8(s + rng.normal(0, 6, s.shape)), u8(0.8 * s + 12 + rng.normal(0, 9, s.shape))
    out["smooth"] = (a, b, 0)
    out["smooth_crop4"] = (a, b, 4)
    x = rng.integers(0, 2, (40, 56, 3))
    out["max1"] = (u8(x), u8(np.where(rng.random(x.shape) < 0.2, 1 - x, x)), 0)           # img1.max() <= 1: max_value = 1
    out["identical"] = (a[:64, :80].copy(), a[:64, :80].copy(), 0)
    bs = np.stack([smooth(rng, 48, 64, 40.0 + 8 * i, 30.0) for i in range(5)])
    out["batch"] = (u8(bs + rng.normal(0, 15, bs.shape)), u8(bs * np.linspace(0.7, 1.1, 5).reshape(5, 1, 1, 1) + rng.normal(0, 18, bs.shape)), 0)
    return out


REF_ERR_MAX = 5e-6      # a quarter of the project's 3-D SSIM bound (2e-5): the bound is to test the kernel, not the reference's rounding


def ssim3d_float64(a, b, border):
    """the 3-D SSIM of two uint8 HWC images in float64 (the window applied axis by axis, which in float64 is the 1331-tap sum to 1e-15):
    the yardstick for the reference's own float32 error on an input"""
    import torch.nn.functional as F
    h, w, _ = a.shape
    x, y = (torch.from_numpy(t[border:h - border, border:w - border].astype(np.float64)) for t in (a, b))
    i = torch.arange(11, dtype=torch.float64) - 5.0
    k = torch.exp(-(i * i) / (2.0 * 1.5 * 1.5))
    k = k / k.sum()

    def window(t):                                                                                   # (H, W, C) volume, replicate padding
        for axis in range(3):
            t = t.movedim(axis, -1)
            s = t.shape
            t = F.conv1d(F.pad(t.reshape(-1, 1, s[-1]), (5, 5), mode="replicate"), k.view(1, 1, 11)).reshape(s).movedim(-1, axis)
        return t
    L = 1 if x.max() <= 1 else 255
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    mu1, mu2 = window(x), window(y)
    s1, s2, s12 = window(x * x) - mu1 * mu1, window(y * y) - mu2 * mu2, window(x * y) - mu1 * mu2
    return float((((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))).mean())


def main():
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    R = reference_functions()
    out, cases = {}, {}
    for name, (a, b, border) in pairs().items():
        xs, ys = (a, b) if a.ndim == 4 else (a[None], b[None])
        psnr = [float(R["calculate_psnr"](x, y, border, input_order="HWC")) for x, y in zip(xs, ys)]
        ssim = [float(R["calculate_ssim"](x, y, border, input_order="HWC", ssim3d=True)) for x, y in zip(xs, ys)]
        ref_err = [abs(s - ssim3d_float64(x, y, border)) for s, x, y in zip(ssim, xs, ys)]
        assert max(ref_err) <= REF_ERR_MAX, f"{name}: the reference's own float32 error is {max(ref_err):.1e}; choose another input"
        out[name + "_x"], out[name + "_y"] = a, b
        cases[name] = {"crop_border": border, "psnr": psnr, "ssim": ssim, "ssim_ref_err": ref_err}
        print(name, a.shape, cases[name])
    out["cases_json"] = np.frombuffer(json.dumps(cases).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(HERE, "paired.npz"), **out)


if __name__ == "__main__":
    main()
