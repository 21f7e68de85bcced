"""GPU: paired evaluation (fdn_hip.metrics.calculate_psnr_ssim_u8, fdn_hip.harness.gt_ratio / validate_u8, calculate_psnr_ssim.py and
validate_fdn.py) against the reference-generated fixture tests/golden/paired.npz and the in-repo oracle.  Tolerances are the project's:
PSNR 1e-9 dB and 3-D SSIM 2e-5 (test_gpu_parity.py::test_metrics_kernels), Y-channel PSNR 1e-5 dB, Y-channel and 2-D SSIM 1e-10 (the
same test), the ratio at rtol 3e-5 (test_gpu_lolv1.py::test_lolv1_harness_u8).  The inputs are textured (random bytes, or waves
with noise at moderate brightness): on flat bright images the reference's own float32 3-D SSIM is rounding-limited
(tests/golden/make_golden_paired.py)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import fdn_oracle as O
from common import fdn_weights, lpnet_weights
from test_paired_cpu import chw, paired_cases

from common import poison_uninitialized  # noqa: F401  (autouse, tests/common.py: torch.empty is filled with NaN / the integer maximum)
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fdn-tip2025_amd")


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import fdn_hip
    fdn_hip.lib()   # fail loudly if the HIP extension is not built
    from fdn_hip import metrics
    return metrics


def cuda(a):
    return (torch.from_numpy(a) if isinstance(a, np.ndarray) else a).to("cuda:0").contiguous()


def load(mod, sd):
    mod.load_state_dict(sd, strict=True)
    return mod.to("cuda:0").eval()


def textured(h, w, seed, n=None):
    """random bytes and a perturbed copy: (img1, img2) uint8 [h][w][3], or [n][h][w][3]"""
    g = np.random.default_rng(seed)
    shape = (h, w, 3) if n is None else (n, h, w, 3)
    a = g.integers(0, 256, shape)
    b = np.clip(a + g.integers(-25, 26, shape), 0, 255)
    return a.astype(np.uint8), b.astype(np.uint8)


def same_psnr(got, want, tol):
    return got == want if want == float("inf") else abs(got - want) < tol


def test_fixture_cases(M):
    """every case of the reference-generated fixture; the five-pair batch in one call, and from host arrays as well as device tensors"""
    for name, a, b, cb, psnr, ssim in paired_cases():
        single = a.shape[0] == 1
        x, y = (a[0], b[0]) if single else (a, b)
        for ins in ((cuda(x), cuda(y)), (x, y)):
            p, s = M.calculate_psnr_ssim_u8(*ins, crop_border=cb)
            p, s = ([p], [s]) if single else (p, s)
            assert len(p) == len(s) == a.shape[0]
            for i in range(a.shape[0]):
                print(f"{name}[{i}]: PSNR {p[i]!r} (ref {psnr[i]!r})  SSIM {s[i]!r} (ref {ssim[i]!r}, diff {s[i] - ssim[i]:+.2e})")
                assert same_psnr(p[i], psnr[i], 1e-9), (name, i, p[i], psnr[i])
                assert abs(s[i] - ssim[i]) < 2e-5, (name, i, s[i], ssim[i])
    name, a, b, cb, psnr, ssim = next(c for c in paired_cases() if c[0] == "identical")
    p, s = M.calculate_psnr_ssim_u8(cuda(a[0]), cuda(b[0]))
    assert p == float("inf") and s == 1.0                                                           # psnr_ssim.py:60-61


def test_batch_equals_single_calls_and_repeats_bit_for_bit(M):
    name, a, b, cb, _, _ = next(c for c in paired_cases() if c[0] == "batch")
    ad, bd = cuda(a), cuda(b)
    p, s = M.calculate_psnr_ssim_u8(ad, bd)
    assert (p, s) == M.calculate_psnr_ssim_u8(ad, bd)                                                # a repeated call
    for i in range(a.shape[0]):
        assert (p[i], s[i]) == M.calculate_psnr_ssim_u8(ad[i], bd[i]), i                             # alone
    order = [3, 0, 4]                                                                                # other neighbours, another place
    p2, s2 = M.calculate_psnr_ssim_u8(ad[order], bd[order])
    assert p2 == [p[i] for i in order] and s2 == [s[i] for i in order]
    x, y = textured(300, 500, seed=11, n=3)                                                          # many tiles: the fixed-order sums
    first = M.calculate_psnr_ssim_u8(cuda(x), cuda(y), crop_border=3)
    for _ in range(3):
        assert M.calculate_psnr_ssim_u8(cuda(x), cuda(y), crop_border=3) == first
    assert M.calculate_psnr_ssim_u8(cuda(x[1]), cuda(y[1]), crop_border=3) == (first[0][1], first[1][1])


@pytest.mark.parametrize("h,w,cb", [(6, 7, 0), (33, 65, 0), (70, 90, 0), (70, 90, 7), (96, 160, 0), (720, 1280, 0)])
def test_sizes_that_do_not_fill_tiles(M, h, w, cb):
    """32 x 32 tiles with a 5-pixel apron: images smaller than the apron, one pixel past a tile, a crop that moves the border, a frame"""
    a, b = textured(h, w, seed=h * 1000 + w + cb)
    p, s = M.calculate_psnr_ssim_u8(cuda(a), cuda(b), crop_border=cb)
    want_p, want_s = O.calculate_psnr(chw(a), chw(b), cb), O.ssim_3d(chw(a), chw(b), cb)
    print(f"{h}x{w} crop {cb}: PSNR {p!r} (oracle {want_p!r})  SSIM {s!r} (oracle {want_s!r}, diff {s - want_s:+.2e})")
    assert abs(p - want_p) < 1e-9
    assert abs(s - want_s) < 2e-5


def test_y_channel_and_2d_branches(M):
    for name, a, b, cb, _, _ in paired_cases():
        if name not in ("smooth_crop4", "batch", "noise"):
            continue
        single = a.shape[0] == 1
        x, y = (cuda(a[0]), cuda(b[0])) if single else (cuda(a), cuda(b))
        py, sy = M.calculate_psnr_ssim_u8(x, y, crop_border=cb, test_y_channel=True)                 # channels B, G, R
        pr, sr = M.calculate_psnr_ssim_u8(x.flip(-1), y.flip(-1), crop_border=cb, test_y_channel=True, bgr=False)
        p2, s2 = M.calculate_psnr_ssim_u8(x, y, crop_border=cb, ssim3d=False)
        # the flip picks the same channels; this branch sums with floating-point atomics, so its own tolerances and no bit equality
        for g_, r_, tol in ((py, pr, 1e-5), (sy, sr, 1e-10)):
            assert all(abs(u - v) < tol for u, v in zip(*(([g_], [r_]) if single else (g_, r_)))), name
        for i in range(a.shape[0]):
            u, v = chw(a[i]), chw(b[i])
            g = (lambda t: t) if single else (lambda t: t[i])
            assert abs(g(py) - O.psnr_y(u, v, cb)) < 1e-5, (name, i)
            assert abs(g(sy) - O.ssim_y(u, v, cb)) < 1e-10, (name, i)
            assert abs(g(p2) - O.calculate_psnr(u, v, cb)) < 1e-9, (name, i)
            assert abs(g(s2) - O.ssim_2d(u, v, cb)) < 1e-10, (name, i)


def test_gt_ratio(M):
    """mean(gray(lq)) / mean(gray(gt)) on the reflect-padded tensors, the reference's op order restated with torch on the CPU
    (image_restoration_model.py:583-586, :650-654; Grayscale = 0.2989 R + 0.587 G + 0.114 B)"""
    import torch.nn.functional as F
    from fdn_hip import FdnHipError, harness
    g = torch.Generator().manual_seed(4)
    gt = torch.randint(0, 256, (3, 40, 72, 3), generator=g, dtype=torch.uint8)
    lq = (gt.float() * torch.tensor([0.08, 0.2, 0.45]).view(3, 1, 1, 1) + torch.randint(0, 6, gt.shape, generator=g)).clamp(0, 255).to(torch.uint8)
    x_lq, h, w = harness.preprocess(cuda(lq), bgr=False)
    x_gt, _, _ = harness.preprocess(cuda(gt), bgr=False)
    got = harness.gt_ratio(x_lq, x_gt)
    assert got.shape == (3, 1) and got.dtype == torch.float32

    def gray_mean(u8):
        t = F.pad(u8.permute(0, 3, 1, 2).float() / 255., (0, 96 - w, 0, 64 - h), mode="reflect")
        gray = 0.2989 * t[:, 0:1] + 0.587 * t[:, 1:2] + 0.114 * t[:, 2:3]
        return torch.mean(gray, dim=(2, 3))
    want = gray_mean(lq) / gray_mean(gt)
    print("gt_ratio", got.cpu().reshape(-1).tolist(), "restated", want.reshape(-1).tolist())
    assert torch.allclose(got.cpu(), want, rtol=3e-5, atol=0)
    assert want.max() / want.min() > 3                                                               # different brightness per image
    with pytest.raises(FdnHipError, match="gray mean 0"):
        harness.gt_ratio(x_lq, torch.zeros_like(x_gt))


@pytest.fixture(scope="module")
def frames():
    g = torch.Generator().manual_seed(6)
    gt = (torch.rand(3, 40, 72, 3, generator=g) * 255).to(torch.uint8)
    lq = (gt.float() * torch.tensor([0.3, 0.45, 0.6]).view(3, 1, 1, 1) + torch.randint(0, 8, gt.shape, generator=g)).clamp(0, 255).to(torch.uint8)
    return lq.numpy(), gt.numpy()


def test_validate_u8(M, frames):
    from basicsr.models.archs.FDN_arch import FDN
    from basicsr.models.archs.LPNet_arch import I_predict_net
    from fdn_hip import harness
    net, lp = load(FDN(), fdn_weights(tame=0.03)), load(I_predict_net(), lpnet_weights())
    lq, gt = cuda(frames[0]), cuda(frames[1])
    out, psnr, ssim, ratio = harness.validate_u8(net, None, lq, gt, ratio_mode="gt", crop_border=2, bgr=False)
    want_ratio = harness.gt_ratio(harness.preprocess(lq, bgr=False)[0], harness.preprocess(gt, bgr=False)[0])
    assert torch.equal(ratio, want_ratio) and ratio.shape == (3, 1)
    want = harness.enhance_u8(net, None, lq, bgr=False, ratio_mode="fixed", ratio=want_ratio)
    assert out.dtype == torch.uint8 and out.shape == gt.shape and torch.equal(out, want)
    assert (psnr, ssim) == M.calculate_psnr_ssim_u8(out, gt, crop_border=2)
    assert len(psnr) == 3 and all(np.isfinite(psnr)) and all(-1 <= s <= 1 for s in ssim)
    # the LPNet ratios, as enhance_u8 feeds them (eager forward)
    for mode in ("lolblur", "lolv1"):
        out, psnr, ssim, ratio = harness.validate_u8(net, lp, lq, gt, ratio_mode=mode, bgr=False)
        want = harness.enhance_u8(net, None, lq, bgr=False, ratio_mode="fixed", ratio=ratio)
        assert torch.equal(out, want), mode
        assert (psnr, ssim) == M.calculate_psnr_ssim_u8(out, gt), mode
    x = harness.preprocess(lq, bgr=False)[0]
    with torch.no_grad():
        assert torch.equal(ratio, harness.lolv1_ratio(x, lp(x)))


def _run(script, *args):
    out = subprocess.run([sys.executable, os.path.join(PKG, script), *args], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stderr
    return out.stdout


LINE = re.compile(r"^ *(\d+): (\S+) *\. \tPSNR: (\S+) dB, \tSSIM: (\S+)$", re.M)
AVERAGE = re.compile(r"^Average: PSNR: (\S+) dB, SSIM: (\S+)$", re.M)


def test_command_lines(M, frames, tmp_path):
    """calculate_psnr_ssim.py and validate_fdn.py on a folder of PNGs: the printed values are the library's, the written frames
    validate_u8's"""
    from PIL import Image
    from basicsr.models.archs.FDN_arch import FDN
    from fdn_hip import harness
    lq, gt = frames
    small = textured(24, 40, seed=2)                                                                 # a pair of another size: its own batch
    for d in ("lq", "gt", "rs"):
        (tmp_path / d).mkdir()
    restored = [np.clip(g.astype(np.int32) + 9 * (i + 1), 0, 255).astype(np.uint8) for i, g in enumerate(gt)]
    for i in range(3):
        Image.fromarray(lq[i]).save(tmp_path / "lq" / f"f{i}.png")
        Image.fromarray(gt[i]).save(tmp_path / "gt" / f"f{i}.png")
        Image.fromarray(restored[i]).save(tmp_path / "rs" / f"f{i}_FDN.png")
    Image.fromarray(small[0]).save(tmp_path / "gt" / "f3.png")
    Image.fromarray(small[1]).save(tmp_path / "rs" / "f3_FDN.png")

    # scoring: ground truth is img1, as in the reference script
    for extra, kw in (([], {}), (["--crop_border", "4"], {"crop_border": 4}), (["--test_y_channel"], {"test_y_channel": True})):
        text = _run("calculate_psnr_ssim.py", "--gt", str(tmp_path / "gt" / "*.png"), "--restored", str(tmp_path / "rs" / "*.png"),
                    "--batch", "2", *extra)
        assert ("Testing Y channel." if kw.get("test_y_channel") else "Testing RGB channels.") in text
        rows = LINE.findall(text)
        assert [r[1] for r in rows] == ["f0", "f1", "f2", "f3"]
        want = [M.calculate_psnr_ssim_u8(cuda(a), cuda(b), bgr=False, **kw) for a, b in list(zip(gt, restored)) + [small]]
        avg = AVERAGE.search(text)
        if kw.get("test_y_channel"):                # this branch sums with floating-point atomics: the printed digits, not the bits
            for (_, _, p, s), (wp, ws) in zip(rows, want):
                assert abs(float(p) - wp) < 1e-6 and abs(float(s) - ws) < 1e-6
            assert abs(float(avg.group(1)) - sum(w[0] for w in want) / 4) < 1e-6 and abs(float(avg.group(2)) - sum(w[1] for w in want) / 4) < 1e-6
        else:
            for (_, _, p, s), (wp, ws) in zip(rows, want):
                assert p == f"{wp:.6f}" and s == f"{ws:.6f}"
            assert avg.group(1) == f"{sum(w[0] for w in want) / 4:.6f}" and avg.group(2) == f"{sum(w[1] for w in want) / 4:.6f}"

    # inference and scoring in one pass
    torch.save({"params": fdn_weights(tame=0.03)}, tmp_path / "fdn.pth")
    text = _run("validate_fdn.py", "--fdn", str(tmp_path / "fdn.pth"), "--lq", str(tmp_path / "lq" / "*.png"), "--gt", str(tmp_path / "gt" / "f[012].png"),
                "--crop_border", "2", "--batch", "2", "--output", str(tmp_path / "out"), "--csv", str(tmp_path / "scores.csv"))
    net = load(FDN(), fdn_weights(tame=0.03))
    out, psnr, ssim, ratio = harness.validate_u8(net, None, cuda(lq), cuda(gt), ratio_mode="gt", crop_border=2, bgr=False)
    rows = LINE.findall(text)
    assert [(r[1], r[2], r[3]) for r in rows] == [(f"f{i}", f"{psnr[i]:.6f}", f"{ssim[i]:.6f}") for i in range(3)]
    assert AVERAGE.search(text).groups() == (f"{sum(psnr) / 3:.6f}", f"{sum(ssim) / 3:.6f}")
    for i in range(3):
        assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / f"f{i}.png")), out[i].cpu().numpy())
    csv = (tmp_path / "scores.csv").read_text().splitlines()
    assert csv[0] == "frame,psnr,ssim,ratio" and len(csv) == 4
    for i, line in enumerate(csv[1:]):
        f, p, s, r = line.rsplit(",", 3)
        assert f.endswith(f"f{i}.png") and float(p) == psnr[i] and float(s) == ssim[i] and float(r) == ratio[i, 0].item()
    # without --output nothing is written
    text2 = _run("validate_fdn.py", "--fdn", str(tmp_path / "fdn.pth"), "--lq", str(tmp_path / "lq" / "*.png"), "--gt", str(tmp_path / "gt" / "f[012].png"),
                 "--crop_border", "2", "--batch", "3")
    assert LINE.findall(text2) == rows and "frames ->" not in text2
    assert sorted(os.listdir(tmp_path)) == ["fdn.pth", "gt", "lq", "out", "rs", "scores.csv"]
