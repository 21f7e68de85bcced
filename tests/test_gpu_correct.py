"""GPU: the brightness-corrected PSNR / SSIM (fdn_hip.correct, csrc/correct.hip in libfdn_correct.so, harness.validate_u8(correct=...),
calculate_psnr_ssim.py --correct and validate_fdn.py --correct) against the float64 truth of tests/correct_ref.py and the in-repo oracle.

The corrected image is held bit for bit: every operation is a correctly rounded double operation on coefficients the host supplied.
The other bounds are the project's own for the same sums and maps (tests/test_gpu_paired.py): PSNR 1e-9 dB against the truth, 3-D SSIM
2e-5 against the oracle on (gt, truth z); the Y-channel and 2-D branches 1e-5 dB, 1e-10 and 1e-10 against the oracle's psnr_y, ssim_y and
ssim_2d on z.  Shapes: smaller than the window and a tile, one past the tile edges, a crop that moves the border, several tiles, and a
batch whose images differ in brightness per image and per channel.  Conditions on the inputs (asserted on the truth, not tolerances):
z stays inside [-64, 320]; and the inputs are strongly textured, so that the oracle's float32 SSIM map is not itself rounding-limited
at the bound it is compared at (tests/test_correct_cpu.py::test_gpu_inputs_are_well_conditioned holds them to that; on the smoother 6 x 7
pair first tried, the oracle's float32 value lay 3.6e-5 from the float64 map and the kernel 1e-6 from it)."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import correct_ref as ref
import fdn_oracle as O
from common import fdn_weights

from common import poison_uninitialized  # noqa: F401  (autouse, tests/common.py: torch.empty is filled with NaN / the integer maximum)
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fdn-tip2025_amd")
MODES = ("gt_mean", "mean_var")
SHAPES = ref.GPU_SHAPES


@pytest.fixture(scope="module")
def C():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import fdn_hip
    fdn_hip.lib()   # fail loudly if the HIP extension is not built
    from fdn_hip import correct
    correct.lib()
    return correct


def cuda(a):
    return (torch.from_numpy(a) if isinstance(a, np.ndarray) else a).to("cuda:0").contiguous()


def chw(a):
    return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))


_truth = {}


def case(shape):
    """(gt, restored, {mode: truth z float32 [h][w][3]}) of a shape of SHAPES, computed once"""
    if shape not in _truth:
        gt, rs = ref.gpu_case(shape)
        z = {m: ref.corrected(gt, rs, m) for m in MODES}
        for m in MODES:
            assert np.isfinite(z[m]).all() and z[m].min() >= -64 and z[m].max() <= 320, (shape, m)      # the input condition
        _truth[shape] = (gt, rs, z)
    return _truth[shape]


def batch3():
    """three 33 x 65 pairs that differ in brightness per image and (ref.textured) per channel"""
    if "batch" not in _truth:
        gt, rs = ref.gpu_batch()
        z = {m: [ref.corrected(a, b, m) for a, b in zip(gt, rs)] for m in MODES}
        for m in MODES:
            assert all(np.isfinite(v).all() and v.min() >= -64 and v.max() <= 320 for v in z[m])
        _truth["batch"] = (gt, rs, z)
    return _truth["batch"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_corrected_image_bit_for_bit(C, shape, mode):
    gt, rs, z = case(shape)
    got = C.corrected_u8(cuda(gt), cuda(rs), mode)
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, 3, shape[0], shape[1])
    got = got[0].permute(1, 2, 0).cpu().numpy()
    diff = np.argwhere(bits(got) != bits(z[mode]))
    assert diff.size == 0, (len(diff), diff[:3], got[tuple(diff[0])], z[mode][tuple(diff[0])])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_scores_against_the_truth(C, shape, mode):
    gt, rs, z = case(shape)
    cb = shape[2]
    p, s = C.calculate_psnr_ssim_corrected_u8(cuda(gt), cuda(rs), mode, crop_border=cb)
    want_p, want_s = ref.psnr(gt, z[mode], cb), O.ssim_3d(chw(gt), chw(z[mode]), cb)
    print(f"{shape} {mode}: PSNR {p!r} (truth {want_p!r}, diff {p - want_p:+.2e})  SSIM {s!r} (oracle {want_s!r}, diff {s - want_s:+.2e})")
    assert abs(p - want_p) < 1e-9
    assert abs(s - want_s) < 2e-5
    # host arrays are moved to the device as calculate_psnr_ssim_u8 moves them: the same bits
    assert (p, s) == C.calculate_psnr_ssim_corrected_u8(gt, rs, mode, crop_border=cb)


@pytest.mark.parametrize("mode", MODES)
def test_y_channel_and_2d_branches(C, mode):
    for shape in ((33, 65, 0), (70, 90, 7)):
        gt, rs, z = case(shape)
        cb = shape[2]
        u, v = chw(gt).float(), chw(z[mode])
        py, sy = C.calculate_psnr_ssim_corrected_u8(cuda(gt), cuda(rs), mode, crop_border=cb, test_y_channel=True)      # channels B, G, R
        p2, s2 = C.calculate_psnr_ssim_corrected_u8(cuda(gt), cuda(rs), mode, crop_border=cb, ssim3d=False)
        print(f"{shape} {mode}: Y PSNR {py!r} SSIM {sy!r}; 2-D PSNR {p2!r} SSIM {s2!r}")
        assert abs(py - O.psnr_y(u, v, cb)) < 1e-5
        assert abs(sy - O.ssim_y(u, v, cb)) < 1e-10
        assert abs(p2 - ref.psnr(gt, z[mode], cb)) < 1e-9
        assert abs(s2 - O.ssim_2d(u, v, cb)) < 1e-10
        # the same pixels handed over as R, G, B
        gf, rf = np.ascontiguousarray(gt[:, :, ::-1]), np.ascontiguousarray(rs[:, :, ::-1])
        pr, sr = C.calculate_psnr_ssim_corrected_u8(cuda(gf), cuda(rf), mode, crop_border=cb, test_y_channel=True, bgr=False)
        assert abs(pr - py) < 1e-5 and abs(sr - sy) < 1e-10


@pytest.mark.parametrize("mode", MODES)
def test_batch_equals_single_calls_and_repeats_bit_for_bit(C, mode):
    gt, rs, z = batch3()
    gd, rd = cuda(gt), cuda(rs)
    p, s = C.calculate_psnr_ssim_corrected_u8(gd, rd, mode)
    assert len(p) == len(s) == 3
    assert (p, s) == C.calculate_psnr_ssim_corrected_u8(gd, rd, mode)                                # a repeated call
    planes = C.corrected_u8(gd, rd, mode)
    for i in range(3):
        assert (p[i], s[i]) == C.calculate_psnr_ssim_corrected_u8(gd[i], rd[i], mode), i             # alone
        assert abs(p[i] - ref.psnr(gt[i], z[mode][i])) < 1e-9, i                                     # its own coefficients, not a neighbour's
        assert abs(s[i] - O.ssim_3d(chw(gt[i]), chw(z[mode][i]))) < 2e-5, i
        assert np.array_equal(bits(planes[i].permute(1, 2, 0).cpu().numpy()), bits(z[mode][i])), i
    order = [2, 0]                                                                                   # other neighbours, another place
    p2, s2 = C.calculate_psnr_ssim_corrected_u8(gd[order], rd[order], mode)
    assert p2 == [p[i] for i in order] and s2 == [s[i] for i in order]
    assert len({round(v, 3) for v in p}) == 3
    if mode == "gt_mean":                                                                            # gray depends on the channel order
        pr, _ = C.calculate_psnr_ssim_corrected_u8(gd, rd, mode, bgr=False)
        assert pr != p and abs(pr[0] - ref.psnr(gt[0], ref.corrected(gt[0], rs[0], mode, bgr=False))) < 1e-9


def test_equal_images_and_a_halved_image(C):
    from fdn_hip import metrics
    gt, _, _ = case((70, 90, 7))
    for mode in MODES:
        p, s = C.calculate_psnr_ssim_corrected_u8(cuda(gt), cuda(gt), mode, crop_border=7)
        assert p == math.inf and abs(s - 1.0) < 2e-5, (mode, p, s)
    half = gt // 2
    plain, _ = metrics.calculate_psnr_ssim_u8(cuda(gt), cuda(half))
    p, _ = C.calculate_psnr_ssim_corrected_u8(cuda(gt), cuda(half), "gt_mean")
    print(f"gt // 2: plain {plain:.3f} dB, gt_mean {p:.3f} dB")
    assert p > plain + 20
    # a ground truth of zeros and ones: the peak value and the SSIM constants are those of 1
    g = np.random.default_rng(5)
    tiny = g.integers(0, 2, (20, 24, 3), dtype=np.uint8)
    noisy = (tiny * 3 + g.integers(0, 3, tiny.shape)).astype(np.uint8)
    for mode in MODES:
        z = ref.corrected(tiny, noisy, mode)
        p, s = C.calculate_psnr_ssim_corrected_u8(cuda(tiny), cuda(noisy), mode)
        assert abs(p - ref.psnr(tiny, z)) < 1e-9 and abs(s - O.ssim_3d(chw(tiny), chw(z))) < 2e-5, mode


def test_degenerate_image_is_nan_alone(C):
    gt, rs, _ = batch3()
    flat = rs.copy()
    flat[1, :, :, 2] = 77
    p, s = C.calculate_psnr_ssim_corrected_u8(cuda(gt), cuda(flat), "mean_var")
    assert math.isnan(p[1]) and math.isnan(s[1])
    for i in (0, 2):
        assert math.isfinite(p[i]) and math.isfinite(s[i])
        assert (p[i], s[i]) == C.calculate_psnr_ssim_corrected_u8(cuda(gt[i]), cuda(flat[i]), "mean_var")
    py, sy = C.calculate_psnr_ssim_corrected_u8(cuda(gt), cuda(flat), "mean_var", test_y_channel=True)
    assert math.isnan(py[1]) and math.isnan(sy[1]) and all(math.isfinite(v) for i in (0, 2) for v in (py[i], sy[i]))
    z = C.corrected_u8(cuda(gt), cuda(flat), "mean_var")
    assert torch.isnan(z[1, 2]).all() and torch.isfinite(z[1, :2]).all() and torch.isfinite(z[0]).all() and torch.isfinite(z[2]).all()
    black = rs.copy()
    black[1] = 0
    p, s = C.calculate_psnr_ssim_corrected_u8(cuda(gt), cuda(black), "gt_mean")
    assert math.isnan(p[1]) and math.isnan(s[1]) and all(math.isfinite(v) for i in (0, 2) for v in (p[i], s[i]))
    # a flat restored image has a gt_mean correction
    p, s = C.calculate_psnr_ssim_corrected_u8(cuda(gt), cuda(flat), "gt_mean")
    assert all(math.isfinite(v) for v in p + s)


@pytest.fixture(scope="module")
def frames():
    g = torch.Generator().manual_seed(8)
    gt = (torch.rand(2, 64, 64, 3, generator=g) * 255).to(torch.uint8)
    lq = (gt.float() * torch.tensor([0.3, 0.5]).view(2, 1, 1, 1) + torch.randint(0, 8, gt.shape, generator=g)).clamp(0, 255).to(torch.uint8)
    return lq.numpy(), gt.numpy()


def test_validate_u8_with_a_correction(C, frames):
    from basicsr.models.archs.FDN_arch import FDN
    from fdn_hip import harness
    net = FDN()
    net.load_state_dict(fdn_weights(tame=0.03), strict=True)
    net = net.to("cuda:0").eval()
    lq, gt = cuda(frames[0]), cuda(frames[1])
    plain = harness.validate_u8(net, None, lq, gt, ratio_mode="gt", crop_border=2, bgr=False)
    both = harness.validate_u8(net, None, lq, gt, ratio_mode="gt", crop_border=2, bgr=False, correct="gt_mean")
    assert len(plain) == 4 and len(both) == 6
    assert torch.equal(plain[0], both[0]) and plain[1] == both[1] and plain[2] == both[2] and torch.equal(plain[3], both[3])
    assert (both[4], both[5]) == C.calculate_psnr_ssim_corrected_u8(gt, both[0], "gt_mean", crop_border=2, bgr=False)
    assert len(both[4]) == 2 and all(math.isfinite(v) for v in both[4] + both[5])


def _run(script, *args):
    out = subprocess.run([sys.executable, os.path.join(PKG, script), *args], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stderr
    return out.stdout


LINE = re.compile(r"^ *(\d+): (\S+) *\. \tPSNR: (\S+) dB, \tSSIM: (\S+?)(?:, \t(\w+) PSNR: (\S+) dB, \t\w+ SSIM: (\S+))?$", re.M)


def test_command_lines(C, tmp_path):
    """each command line once, as a child process, on a folder of four PNGs: 16 x 20 for the scorer; 20 x 24 for validate_fdn.py, whose
    reflect padding to the x32 grid needs pad < size and so refuses 16 rows"""
    from PIL import Image
    from basicsr.models.archs.FDN_arch import FDN
    from fdn_hip import harness
    for d in ("gt", "rs", "vgt", "vlq"):
        (tmp_path / d).mkdir()
    pairs = [ref.textured(16, 20, seed=60 + i, gain=g) for i, g in enumerate((0.5, 0.8, 1.2, 1.6))]
    for i, (a, b) in enumerate(pairs):
        Image.fromarray(a).save(tmp_path / "gt" / f"f{i}.png")
        Image.fromarray(b).save(tmp_path / "rs" / f"f{i}.png")
    text = _run("calculate_psnr_ssim.py", "--gt", str(tmp_path / "gt" / "*.png"), "--restored", str(tmp_path / "rs" / "*.png"),
                "--correct", "mean_var", "--crop_border", "1", "--batch", "3")
    assert "Testing RGB channels. Correction: mean_var." in text
    rows = LINE.findall(text)
    want = [C.calculate_psnr_ssim_corrected_u8(cuda(a), cuda(b), "mean_var", crop_border=1, bgr=False) for a, b in pairs]
    assert [(r[1], r[2], r[3]) for r in rows] == [(f"f{i}", f"{p:.6f}", f"{s:.6f}") for i, (p, s) in enumerate(want)]

    vp = [ref.textured(20, 24, seed=70 + i, gain=0.4, offset=4.0) for i in range(4)]
    for i, (a, b) in enumerate(vp):
        Image.fromarray(a).save(tmp_path / "vgt" / f"f{i}.png")
        Image.fromarray(b).save(tmp_path / "vlq" / f"f{i}.png")
    torch.save({"params": fdn_weights(tame=0.03)}, tmp_path / "fdn.pth")
    text = _run("validate_fdn.py", "--fdn", str(tmp_path / "fdn.pth"), "--lq", str(tmp_path / "vlq" / "*.png"), "--gt", str(tmp_path / "vgt" / "*.png"),
                "--correct", "gt_mean", "--csv", str(tmp_path / "scores.csv"))
    net = FDN()
    net.load_state_dict(fdn_weights(tame=0.03), strict=True)
    net = net.to("cuda:0").eval()
    gt, lq = cuda(np.stack([p[0] for p in vp])), cuda(np.stack([p[1] for p in vp]))
    out, psnr, ssim, ratio, pc, sc = harness.validate_u8(net, None, lq, gt, ratio_mode="gt", bgr=False, correct="gt_mean")
    rows = LINE.findall(text)
    assert [r[1:] for r in rows] == [(f"f{i}", f"{psnr[i]:.6f}", f"{ssim[i]:.6f}", "gt_mean", f"{pc[i]:.6f}", f"{sc[i]:.6f}") for i in range(4)]
    csv = (tmp_path / "scores.csv").read_text().splitlines()
    assert csv[0] == "frame,psnr,ssim,ratio,psnr_corr,ssim_corr" and len(csv) == 5
    for i, line in enumerate(csv[1:]):
        f, p, s, r, p2, s2 = line.rsplit(",", 5)
        assert f.endswith(f"f{i}.png") and (float(p), float(s), float(p2), float(s2)) == (psnr[i], ssim[i], pc[i], sc[i])
