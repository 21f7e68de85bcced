"""Golden values for the FFT term of the reference's loss (options/train/FDN.yml: L1 + 0.1 FFTLoss): the class FFTLoss and the function
l1_loss it calls are lifted out of the reference's basicsr/models/losses/losses.py by AST (the package route imports cv2, absent here), with
weighted_loss taken from basicsr/models/losses/loss_util.py loaded by path, and run with reduction='mean' on three small 8-bit image pairs
scaled by 1/255: a gain error with strong noise, a pair near 45 dB, and a displaced copy.  Next to every value the fixture stores its
relative distance from the float64 formula (tests/spectral_ref.py fft_l1): the reference computes in float32, and a pair is admitted only
if that distance is at most 1e-5.  Run:  python tests/golden/make_golden_fourier.py"""
import ast
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from _refload import REF_ROOT  # noqa: E402
import spectral_ref  # noqa: E402


def reference_fft_loss():
    losses = os.path.join(REF_ROOT, "basicsr", "models", "losses")
    spec = importlib.util.spec_from_file_location("_ref_loss_util", os.path.join(losses, "loss_util.py"))
    util = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(util)
    path = os.path.join(losses, "losses.py")
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if (isinstance(n, ast.FunctionDef) and n.name == "l1_loss") or (isinstance(n, ast.ClassDef) and n.name == "FFTLoss")]
    ns = {"torch": torch, "nn": torch.nn, "F": torch.nn.functional, "np": np, "weighted_loss": util.weighted_loss,
          "_reduction_modes": ["none", "mean", "sum"]}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns["FFTLoss"](loss_weight=1.0, reduction="mean")


def pairs():
    """(name, restored, ground truth) uint8 [h][w][3]"""
    g = np.random.default_rng(2025)
    gt = spectral_ref.textured(36, 50, seed=11)
    yield "gain_noise", np.clip(np.rint(0.8 * gt + g.normal(0.0, 20.0, gt.shape)), 0, 255).astype(np.uint8), gt
    gt = spectral_ref.textured(45, 64, seed=12)
    yield "near_45db", np.clip(gt.astype(np.int64) + (g.random(gt.shape) < 0.55) * g.integers(-3, 4, gt.shape), 0, 255).astype(np.uint8), gt
    gt = spectral_ref.textured(24, 32, seed=13)
    yield "rolled", np.roll(gt, (3, 5), axis=(0, 1)), gt


def main():
    loss = reference_fft_loss()
    out, cases = {}, {}
    for name, rs, gt in pairs():
        a, b = (torch.from_numpy(x).permute(2, 0, 1).unsqueeze(0).float() / 255.0 for x in (rs, gt))
        value = float(loss(a, b))
        exact = spectral_ref.fft_l1(a[0].double().numpy(), b[0].double().numpy())
        dist = abs(value - exact) / exact
        psnr = 10 * np.log10(1.0 / float(((a.double() - b.double()) ** 2).mean()))
        print(f"{name}: FFTLoss {value!r}  float64 formula {exact!r}  relative distance {dist:.3e}  PSNR {psnr:.2f} dB")
        assert dist <= 1e-5, name
        out[name + "_restored"], out[name + "_gt"] = rs, gt
        cases[name] = {"fft_l1": value, "distance": dist}
    out["cases_json"] = np.frombuffer(json.dumps(cases).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(HERE, "fourier.npz"), **out)


if __name__ == "__main__":
    main()
