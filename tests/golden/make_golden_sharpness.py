"""Record tests/golden/sharpness.npz: the reference's own EdgeLoss on small 8-bit image pairs (test tooling; runs only where the reference
checkout is present, and copies nothing from it).

basicsr/models/losses/losses.py is loaded BY PATH (the package route dies on `import cv2`), with `torchvision.models.vgg` and
`basicsr.models.losses.loss_util.weighted_loss` answered by stubs in sys.modules, in the manner of tests/golden/_refload.py: EdgeLoss
(:661-687) and its CharbonnierLoss (:647-658) need neither.  Per case the file holds
    a_<k>, b_<k>   the two byte images [h][w][3] (a: ground truth, b: restored);
    f32_<k>        EdgeLoss()(x, y) as the reference computes it, float32 tensors of a / 255 and b / 255;
    f64_<k>        the reference's formula evaluated by the same module in float64 (its kernel and its inputs cast to double:
                   the weights are then the doubles nearest to float32(.05) .. float32(.4), so part of |f32 - f64| and of the
                   distance to the exact-weights figure is the float32 weights themselves: 0.05f is not 1/20);
    gap            the largest |f32 - f64| over the cases, from which tests/test_sharpness_cpu.py forms its bound.
Cases: 1x1, 2x3, 5x5, 6x7, 7x6, 33x47 and 64x90, each with a blurred and dimmed copy against its source and with two unrelated images.

    python tests/golden/make_golden_sharpness.py"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import sharpness_ref as ref  # noqa: E402

REF_ROOT = os.environ.get("FDN_REFERENCE_ROOT", "/root/reference")
LOSSES = os.path.join(REF_ROOT, "basicsr", "models", "losses", "losses.py")
SIZES = [(1, 1), (2, 3), (5, 5), (6, 7), (7, 6), (33, 47), (64, 90)]


def reference_losses():
    """the reference's losses.py as a module, under the two stubs"""
    stubs = {}
    for name in ("torchvision", "torchvision.models", "torchvision.models.vgg", "basicsr", "basicsr.models", "basicsr.models.losses",
                 "basicsr.models.losses.loss_util"):
        if name not in sys.modules:
            stubs[name] = types.ModuleType(name)
    if "torchvision.models" in stubs:
        stubs["torchvision.models"].vgg = stubs.get("torchvision.models.vgg", sys.modules.get("torchvision.models.vgg"))
    if "basicsr.models.losses.loss_util" in stubs:
        stubs["basicsr.models.losses.loss_util"].weighted_loss = lambda f: f
    sys.modules.update(stubs)
    try:
        spec = importlib.util.spec_from_file_location("_ref_losses", LOSSES)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for name in stubs:
            sys.modules.pop(name, None)
    return mod


def cases():
    for k, (h, w) in enumerate(SIZES):
        yield ref.soft_pair(h, w, seed=100 + k)
        yield ref.random_pair(h, w, seed=200 + k)


def main():
    if not os.path.isfile(LOSSES):
        sys.exit(f"{LOSSES} not found: this script runs only beside the reference checkout")
    loss = reference_losses().EdgeLoss("cpu")
    nchw = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))).to(dt).unsqueeze(0) / 255
    out, gap = {}, 0.0
    for k, (a, b) in enumerate(cases()):
        with torch.no_grad():
            loss.kernel = loss.kernel.float()
            f32 = float(loss(nchw(a, torch.float32), nchw(b, torch.float32)))
            loss.kernel = loss.kernel.double()
            f64 = float(loss(nchw(a, torch.float64), nchw(b, torch.float64)))
        ours = ref.edge_error(a, b)
        print(f"{k:2d} {a.shape[0]:3d}x{a.shape[1]:<3d} reference float32 {f32:.9e}  float64 {f64:.9e}  |f32 - f64| {abs(f32 - f64):.2e}  "
              f"integer form - float64 {ours - f64:+.2e}")
        gap = max(gap, abs(f32 - f64))
        out[f"a_{k}"], out[f"b_{k}"], out[f"f32_{k}"], out[f"f64_{k}"] = a, b, np.float64(f32), np.float64(f64)
    out["gap"] = np.float64(gap)
    print(f"largest |float32 - float64| {gap:.3e}")
    np.savez_compressed(os.path.join(HERE, "sharpness.npz"), **out)


if __name__ == "__main__":
    main()
