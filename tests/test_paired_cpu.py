"""CPU: the paired 8-bit metrics' fixture (tests/golden/make_golden_paired.py) against the oracle, the facts the GPU path rests on (a byte
survives float32 / 255 * 255; the replicate-padded channel pass is a 3 x 3 matrix; W pass, H pass and that matrix in float32 stay inside
the project's 3-D SSIM tolerance), the argument errors that need no device and the pairing of the two command lines.  No GPU."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fdn_oracle as O
from common import GOLDEN

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "fdn-tip2025_amd")


def paired_cases():
    """[(name, img1 uint8 [B][h][w][3], img2, crop_border, [psnr], [ssim])] of paired.npz"""
    z = np.load(os.path.join(GOLDEN, "paired.npz"))
    cases = json.loads(bytes(z["cases_json"]).decode())
    out = []
    for k, v in cases.items():
        a, b = z[k + "_x"], z[k + "_y"]
        if a.ndim == 3:
            a, b = a[None], b[None]
        out.append((k, a, b, v["crop_border"], v["psnr"], v["ssim"]))
    return out


def chw(u):
    return torch.from_numpy(u.astype(np.float32)).permute(2, 0, 1).contiguous()


@pytest.fixture(scope="module")
def clis():
    sys.path.insert(0, PKG)
    import calculate_psnr_ssim
    import validate_fdn
    return calculate_psnr_ssim, validate_fdn


def test_fixture_holds_the_cases_and_small_inputs():
    cases = {c[0]: c for c in paired_cases()}
    assert set(cases) == {"noise", "smooth", "smooth_crop4", "max1", "identical", "batch"}
    for name, a, b, cb, psnr, ssim in cases.values():
        assert a.dtype == b.dtype == np.uint8 and a.shape == b.shape and a.shape[1] <= 96 and a.shape[2] <= 160 and a.shape[3] == 3
        assert len(psnr) == len(ssim) == a.shape[0]
    assert cases["batch"][1].shape[0] == 5 and cases["smooth_crop4"][3] == 4
    assert cases["max1"][1].max() == 1
    assert cases["identical"][4] == [float("inf")] and cases["identical"][5] == [1.0]


def test_fixture_against_the_oracle():
    """the reference's values on uint8 HWC arrays = the oracle's on the float CHW copy, at the bounds of test_oracle_golden.py"""
    for name, a, b, cb, psnr, ssim in paired_cases():
        for i in range(a.shape[0]):
            p = O.calculate_psnr(chw(a[i]), chw(b[i]), cb)
            assert p == psnr[i] if psnr[i] == float("inf") else abs(p - psnr[i]) < 1e-9, (name, i)
            assert abs(O.ssim_3d(chw(a[i]), chw(b[i]), cb) - ssim[i]) < 1e-6, (name, i)


def test_integer_sum_of_squares_gives_the_psnr():
    from fdn_hip.metrics import _psnr_from_sse
    for name, a, b, cb, psnr, _ in paired_cases():
        for i in range(a.shape[0]):
            x, y = (t[i, cb:a.shape[1] - cb, cb:a.shape[2] - cb].astype(np.int64) for t in (a, b))
            got = _psnr_from_sse(int(((x - y) ** 2).sum()), float(x.max()), x.size)
            assert got == psnr[i] if psnr[i] == float("inf") else abs(got - psnr[i]) < 1e-9, (name, i)


def test_a_byte_survives_the_scripts_float32_round_trip():
    """scripts/metrics/calculate_psnr_ssim.py scores float32(byte) / 255. * 255. (:31, :36, :61): the byte again, for every byte"""
    assert np.array_equal((np.arange(256, dtype=np.float32) / 255.) * 255., np.arange(256))


def test_channel_matrix_is_the_replicate_padded_channel_pass():
    from fdn_hip.metrics import ssim3d_channel_matrix, ssim3d_taps
    k, m = ssim3d_taps(), ssim3d_channel_matrix()
    assert k.dtype == np.float64 and torch.equal(torch.from_numpy(k), O.gaussian_kernel_11())
    assert m.shape == (3, 3) and np.allclose(m.sum(axis=1), 1.0, rtol=0, atol=1e-15)
    # the 11 taps over the replicate-padded channel axis, applied to the three unit vectors
    eye = F.pad(torch.eye(3, dtype=torch.float64)[:, None], (5, 5), mode="replicate")               # [c_in][1][13]
    want = F.conv1d(eye, torch.from_numpy(k)[None, None])[:, 0].T                                    # [c_out][c_in]
    assert np.allclose(m, want.numpy(), rtol=0, atol=1e-16)
    assert np.allclose(m, m[::-1, ::-1], rtol=0, atol=1e-15)                                         # symmetric along the channel axis: bgr or rgb


def test_separable_float32_passes_stay_inside_the_3d_ssim_tolerance():
    """the kernel's arithmetic restated with torch on the CPU: W pass, H pass, 3 x 3 channel matrix, all float32, against the reference's
    1331-tap values at the project's 2e-5"""
    from fdn_hip.metrics import ssim3d_channel_matrix, ssim3d_taps
    k = torch.from_numpy(ssim3d_taps()).to(torch.float32)
    m = torch.from_numpy(ssim3d_channel_matrix()).to(torch.float32)

    def window(t):                                                                                   # [3][h][w]
        t = F.conv2d(F.pad(t[:, None], (5, 5, 0, 0), mode="replicate"), k.view(1, 1, 1, 11))
        t = F.conv2d(F.pad(t, (0, 0, 5, 5), mode="replicate"), k.view(1, 1, 11, 1))[:, 0]
        return torch.einsum("oc,chw->ohw", m, t)

    for name, a, b, cb, _, ssim in paired_cases():
        for i in range(a.shape[0]):
            x, y = (chw(t[i])[:, cb:a.shape[1] - cb, cb:a.shape[2] - cb] for t in (a, b))
            L = 1 if x.max() <= 1 else 255
            C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
            mu1, mu2 = window(x), window(y)
            s1, s2, s12 = window(x * x) - mu1 * mu1, window(y * y) - mu2 * mu2, window(x * y) - mu1 * mu2
            got = (((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))).double().mean().item()
            assert abs(got - ssim[i]) < 2e-5, (name, i, got, ssim[i])


def test_argument_errors_that_need_no_device():
    from fdn_hip import FdnHipError, harness, metrics
    z = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(FdnHipError, match=r"Image shapes are different: \(8, 8, 3\), \(8, 9, 3\)\."):
        metrics.calculate_psnr_ssim_u8(z, np.zeros((8, 9, 3), np.uint8))
    with pytest.raises(FdnHipError, match="takes uint8 images"):
        metrics.calculate_psnr_ssim_u8(z.astype(np.float32), z.astype(np.float32))
    with pytest.raises(FdnHipError, match="takes uint8 images"):
        metrics.calculate_psnr_ssim_u8(np.zeros((8, 8, 1), np.uint8), np.zeros((8, 8, 1), np.uint8))
    with pytest.raises(FdnHipError, match="takes uint8 images"):
        metrics.calculate_psnr_ssim_u8(torch.zeros(8, 8, dtype=torch.uint8), torch.zeros(8, 8, dtype=torch.uint8))
    with pytest.raises(FdnHipError, match="nothing is left"):
        metrics.calculate_psnr_ssim_u8(z, z, crop_border=4)
    with pytest.raises(FdnHipError, match="crop_border must be >= 0"):
        metrics.calculate_psnr_ssim_u8(z, z, crop_border=-1)
    with pytest.raises(FdnHipError, match="two \\[B,3,H,W\\] tensors of one shape"):
        harness.gt_ratio(torch.zeros(2, 3, 32, 32), torch.zeros(2, 3, 32, 64))
    with pytest.raises(ValueError, match="ratio_mode 'fixed'"):
        harness.validate_u8(None, None, torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 8, 8, 3, dtype=torch.uint8), ratio_mode="fixed")
    with pytest.raises(FdnHipError, match="ratio_mode 'lolv1' needs lpnet"):
        harness.validate_u8(None, None, torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 8, 8, 3, dtype=torch.uint8), ratio_mode="lolv1")
    with pytest.raises(FdnHipError, match="Image shapes are different"):
        harness.validate_u8(None, None, torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 8, 9, 3, dtype=torch.uint8))


def _png(path, a):
    from PIL import Image
    Image.fromarray(a).save(path)


def _folders(tmp_path, names=("b", "a", "c")):
    g = np.random.default_rng(0)
    gt, rs = tmp_path / "gt", tmp_path / "rs"
    gt.mkdir(); rs.mkdir()
    for n in names:
        _png(gt / f"{n}.png", g.integers(0, 256, (16, 20, 3), dtype=np.uint8))
        _png(rs / f"{n}_out.png", g.integers(0, 256, (16, 20, 3), dtype=np.uint8))
    return gt, rs


def test_scoring_cli_pairs_and_refuses(clis, tmp_path, capsys):
    cli, _ = clis
    gt, rs = _folders(tmp_path)
    assert cli.pair_paths(str(gt / "*.png"), str(rs / "*.png")) == [(str(gt / f"{n}.png"), str(rs / f"{n}_out.png")) for n in "abc"]
    assert cli.group_pairs([((16, 20, 3), (16, 20, 3))] * 3, 2) == [[0, 1], [2]]
    os.remove(rs / "c_out.png")
    for argv in (["--gt", str(gt / "*.png"), "--restored", str(rs / "*.png")],                    # 3 against 2
                 ["--gt", str(tmp_path / "none" / "*.png"), "--restored", str(rs / "*.png")],      # no ground truth
                 ["--gt", str(gt / "[ab].png"), "--restored", str(rs / "*.png"), "--crop_border", "-1"],
                 ["--gt", str(gt / "[ab].png"), "--restored", str(rs / "*.png"), "--correct_mean_var"],
                 ["--restored", str(rs / "*.png")]):
        with pytest.raises(SystemExit):
            cli.main(argv)
    with pytest.raises(SystemExit):
        cli.main(["--help"])
    assert "--correct_mean_var" in capsys.readouterr().out                                           # the help says that it is not offered


def test_cli_decodes_group_by_group(clis, tmp_path):
    """sizes from the headers, groups of one size in order of first appearance, at most one group decoding ahead of the one handed out"""
    from concurrent.futures import ThreadPoolExecutor
    cli, _ = clis
    g = np.random.default_rng(1)
    sizes = [(16, 20), (12, 12), (16, 20), (16, 20), (12, 12)]
    imgs = [(g.integers(0, 256, (h, w, 3), dtype=np.uint8), g.integers(0, 256, (h, w, 3), dtype=np.uint8)) for h, w in sizes]
    pairs = []
    for i, (a, b) in enumerate(imgs):
        _png(tmp_path / f"a{i}.png", a)
        _png(tmp_path / f"b{i}.png", b)
        pairs.append((str(tmp_path / f"a{i}.png"), str(tmp_path / f"b{i}.png")))
    assert cli.image_shape(pairs[1][0]) == (12, 12, 3)

    class Counting(ThreadPoolExecutor):
        submitted = 0

        def submit(self, *a, **k):
            self.submitted += 1
            return super().submit(*a, **k)
    with Counting(max_workers=2) as pool:
        seen = []
        for n, (idx, first, second) in enumerate(cli.decoded_groups(pairs, 2, pool)):
            assert pool.submitted <= 2 * sum(len(i) for i in ([0, 2], [3], [1, 4])[:n + 2])           # this group and the next, no more
            assert all(np.array_equal(first[k], imgs[i][0]) and np.array_equal(second[k], imgs[i][1]) for k, i in enumerate(idx))
            seen.append(idx)
    assert seen == [[0, 2], [3], [1, 4]]
    _png(tmp_path / "b4.png", imgs[0][0])
    with pytest.raises(ValueError, match="differ in size"):
        next(cli.decoded_groups(pairs, 2, None))


def test_validation_cli_pairs_and_refuses(clis, tmp_path):
    _, cli = clis
    gt, lq = _folders(tmp_path)
    assert cli.pair_frames(str(lq / "*.png"), str(gt / "*.png")) == [(str(lq / f"{n}_out.png"), str(gt / f"{n}.png")) for n in "abc"]
    base = ["--fdn", "unused.pth", "--lq", str(lq / "*.png"), "--gt", str(gt / "*.png")]
    a = cli.parse_args(base + ["--output", str(tmp_path / "out")])
    assert (a.ratio, a.variant, a.crop_border, a.batch, a.csv) == ("gt", "lolblur", 0, 8, None)
    assert a.dest == [str(tmp_path / "out" / f"{n}_out.png") for n in "abc"]
    assert cli.parse_args(base).dest is None                                                         # frames are written only with --output
    assert cli.RATIO_MODE[("gt", "lolv1")] == "gt" and cli.RATIO_MODE[("lpnet", "lolblur")] == "lolblur" and cli.RATIO_MODE[("lpnet", "lolv1")] == "lolv1"
    (tmp_path / "s1").mkdir(); (tmp_path / "s2").mkdir()
    assert cli.output_paths([str(tmp_path / "s1" / "0.png"), str(tmp_path / "s2" / "0.png")], "o") == [os.path.join("o", "s1", "0.png"), os.path.join("o", "s2", "0.png")]
    os.remove(gt / "c.png")
    for argv in (base,                                                                              # 3 against 2
                 ["--fdn", "unused.pth", "--lq", str(tmp_path / "none" / "*.png"), "--gt", str(gt / "*.png")],
                 ["--fdn", "unused.pth", "--lq", str(lq / "[ab]*.png"), "--gt", str(gt / "*.png"), "--ratio", "lpnet"],      # no --lpnet
                 ["--fdn", "unused.pth", "--lq", str(lq / "[ab]*.png"), "--gt", str(gt / "*.png"), "--ratio", "fixed"],
                 ["--fdn", "unused.pth", "--lq", str(lq / "[ab]*.png"), "--gt", str(gt / "*.png"), "--crop_border", "-2"],
                 ["--lq", str(lq / "[ab]*.png"), "--gt", str(gt / "*.png")]):
        with pytest.raises(SystemExit):
            cli.parse_args(argv)
