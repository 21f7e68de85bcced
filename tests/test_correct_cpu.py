"""CPU: the host side of the brightness-corrected PSNR / SSIM - the entry points of include/fdn_correct.h in libfdn_correct.so (version,
generated prototype table, every argument refusal before any launch, the workspace query), fdn_hip.correct.correction_coefficients against
the restatement of tests/correct_ref.py, the restatement's single affine map against the reference's float32 two-pass procedure, and the
argument parsing of calculate_psnr_ssim.py --correct and validate_fdn.py --correct.  No GPU compute."""
import ctypes
import importlib.util
import math
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as entry  # noqa: F401  (puts the package on sys.path)
import correct_ref as ref
from fdn_hip import correct  # noqa: E402  (the module under test: without it nothing here has a subject)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fdn-tip2025_amd")
NAMES = ["fdn_correct_abi_version", "fdn_pair_moments_u8", "fdn_pair_moments_fold", "fdn_pair_corrected_ws", "fdn_pair_corrected_u8",
         "fdn_pair_apply_u8"]
# the float32 two-pass procedure of the reference against the single affine map in double, measured with numpy on the five cases of
# test_affine_map_is_the_references_two_passes: the largest PSNR difference and the largest |dz|; the test allows 8 times each
MEASURED_DPSNR, MEASURED_DZ = 2.6e-6, 6.2e-5


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(correct.lib_path()):
        entry.build()
    return correct.lib()


def same(a, b):
    """== on doubles, NaN equal to NaN"""
    return a == b or (math.isnan(a) and math.isnan(b))


def test_version_and_generated_table(lib, monkeypatch):
    spec = importlib.util.spec_from_file_location("gen_abi_table", os.path.join(ROOT, "tools", "gen_abi_table.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    from fdn_hip import _abi_correct as table
    protos, names, members, versions = gen.build_table(headers=["fdn_correct.h"])
    assert table.PROTOTYPES == protos and table.ARG_NAMES == names and list(protos) == members["fdn_correct.h"] == NAMES
    assert table.VERSION == versions["fdn_correct.h"] == ("fdn_correct_abi_version", 1)
    assert "fdn_correct.h" not in gen.HEADERS                                      # the one table of libfdn_hip.so stays what it was
    assert lib.fdn_correct_abi_version() == 1 == correct.ABI_VERSION
    assert lib.fdn_pair_corrected_ws.restype == ctypes.c_long
    assert lib.fdn_pair_corrected_u8.argtypes == [ctypes.c_void_p] * 2 + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 7
    assert table.ARG_NAMES["fdn_pair_corrected_u8"] == ["gt", "restored", "B", "h", "w", "crop", "coef", "is255", "taps11", "chmix9", "ws",
                                                        "out2", "stream"]
    # libfdn_hip.so neither holds these entry points nor depends on the new library
    import fdn_hip
    assert not hasattr(fdn_hip.lib(), "fdn_pair_corrected_u8")
    # a library of another version is refused with the sentence of fdn_hip.lib()
    monkeypatch.setattr(correct, "_lib", None)
    monkeypatch.setattr(correct, "ABI_VERSION", 2)
    with pytest.raises(ImportError, match=r"libfdn_correct\.so has correct ABI version 1, this binding needs 2: rebuild with build\.sh"):
        correct.lib()
    assert correct._lib is None


GOOD = dict(B=2, h=40, w=50, crop=3)
BAD = [dict(B=0), dict(B=-1), dict(B=65536), dict(h=0), dict(h=-4), dict(w=0), dict(w=-1), dict(h=46341, w=46341), dict(h=2 ** 31 - 1, w=2)]
BAD_CROP = [dict(crop=-1), dict(crop=20), dict(crop=25), dict(h=6, crop=3), dict(w=6, crop=3)]


def test_entry_points_validate_arguments_without_gpu(lib):
    """every refusal of include/fdn_correct.h is FDN_ERR_ARG = 1 before any launch (this machine may have no GPU to launch on, and the
    pointers are never dereferenced); the workspace query answers 0 to the same sizes, and otherwise two doubles per tile"""
    p = ctypes.c_void_p(64)                                                        # never dereferenced
    taps = (ctypes.c_double * 11)()
    mix = (ctypes.c_double * 9)()

    def moments(gt=p, rs=p, out=p, **kw):
        a = {**GOOD, **kw}
        return lib.fdn_pair_moments_u8(gt, rs, a["B"], a["h"], a["w"], a["crop"], out, None)

    def corrected(ptrs=None, **kw):
        a = {**GOOD, **kw}
        q = dict(gt=p, rs=p, coef=p, is255=p, taps=taps, mix=mix, ws=p, out=p)
        q.update(ptrs or {})
        return lib.fdn_pair_corrected_u8(q["gt"], q["rs"], a["B"], a["h"], a["w"], a["crop"], q["coef"], q["is255"], q["taps"], q["mix"],
                                         q["ws"], q["out"], None)

    def apply(rs=p, coef=p, out=p, **kw):
        a = {**GOOD, **kw}
        return lib.fdn_pair_apply_u8(rs, coef, a["B"], a["h"], a["w"], out, None)

    def ws(**kw):
        a = {**GOOD, **kw}
        return lib.fdn_pair_corrected_ws(a["B"], a["h"], a["w"], a["crop"])

    for bad in BAD + BAD_CROP:
        assert moments(**bad) == 1, bad
        assert corrected(**bad) == 1, bad
        assert ws(**bad) == 0, bad
    for bad in BAD:
        assert apply(**bad) == 1, bad
    for k in ("gt", "rs", "out"):
        assert moments(**{k: None}) == 1, k
    for k in ("gt", "rs", "coef", "is255", "taps", "mix", "ws", "out"):
        assert corrected({k: None}) == 1, k
    for k in ("rs", "coef", "out"):
        assert apply(**{k: None}) == 1, k
    for args in ((None, 1, p), (p, 1, None), (p, 0, p), (p, -1, p), (p, 65536, p)):
        assert lib.fdn_pair_moments_fold(args[0], args[1], args[2], None) == 1, args
    assert ws() == 2 * 2 * 2 * 2                                                   # 34 x 44 cropped: 2 x 2 tiles of 32 x 32
    assert ws(B=1, h=6, w=7, crop=0) == 2 and ws(B=3, h=33, w=65, crop=0) == 3 * 2 * 3 * 2 and ws(B=1, h=720, w=1280, crop=0) == 2 * 23 * 40
    assert ws(B=65535, h=1, w=2 ** 31 - 1, crop=0) == 2 * 65535 * 2 ** 26


def test_module_refuses_without_a_device():
    from fdn_hip import FdnHipError
    z = np.zeros((8, 8, 3), np.uint8)
    for f in (lambda m: correct.calculate_psnr_ssim_corrected_u8(z, z, m), lambda m: correct.corrected_u8(z, z, m),
              lambda m: correct.correction_coefficients([[0] * 13], m, n=4)):
        for mode in ("mean", None, "correct_mean_var", "GT_MEAN"):
            with pytest.raises(FdnHipError, match="correction mode must be one of gt_mean, mean_var"):
                f(mode)
    with pytest.raises(FdnHipError, match="Image shapes are different"):
        correct.calculate_psnr_ssim_corrected_u8(z, np.zeros((8, 9, 3), np.uint8), "gt_mean")
    with pytest.raises(FdnHipError, match="calculate_psnr_ssim_corrected_u8 takes uint8 images"):
        correct.calculate_psnr_ssim_corrected_u8(z.astype(np.float32), z.astype(np.float32), "gt_mean")
    with pytest.raises(FdnHipError, match="nothing is left"):
        correct.calculate_psnr_ssim_corrected_u8(z, z, "mean_var", crop_border=4)
    with pytest.raises(FdnHipError, match="13 moments"):
        correct.correction_coefficients([[0] * 12], "gt_mean", n=4)
    from fdn_hip import harness
    import torch
    u = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(FdnHipError, match="correction mode must be one of"):
        harness.validate_u8(None, None, u, u, correct="mean")
    src = open(os.path.join(PKG, "fdn_hip", "correct.py")).read()
    assert "oracle" not in src and "tests" not in src.replace("tests/", "")           # the product path stands without the yardsticks


@pytest.mark.parametrize("bgr", [True, False])
def test_coefficients_equal_the_restatement(bgr):
    """Python integers, one division (and one square root) in double: == on every double"""
    for k, (h, w) in enumerate([(6, 7), (33, 65), (70, 90), (96, 160)]):
        gt, rs = ref.textured(h, w, seed=k, gain=(0.5, 1.7, 0.8, 1.2)[k], offset=(20.0, -40.0, 5.0, 0.0)[k])
        for mode in correct.MODES:
            got = correct.correction_coefficients([ref.moments(gt, rs)], mode, bgr, n=h * w)
            want = ref.coefficients(gt, rs, mode, bgr)
            assert len(got) == 1 and all(same(g, x) for gr, wr in zip(got[0], want) for g, x in zip(gr, wr)), (h, w, mode, got, want)
            assert all(0.3 < row[1] < 3 for row in got[0])
        if bgr:
            assert correct.correction_coefficients([ref.moments(gt, rs)], "gt_mean", False, n=h * w) != ref.coefficients(gt, rs, "gt_mean", True)
    # several images: one row each, in order
    pairs = [ref.textured(12, 9, seed=s, gain=g) for s, g in ((5, 0.6), (6, 1.5), (7, 1.0))]
    got = correct.correction_coefficients([ref.moments(a, b) for a, b in pairs], "mean_var", bgr, n=108)
    assert got == [ref.coefficients(a, b, "mean_var", bgr) for a, b in pairs]


def test_sums_of_an_8k_frame_do_not_overflow():
    """an all-255 7680 x 4320 image: the int64 sums of the device hold it, and the host's products are Python integers"""
    h, w = 4320, 7680
    n = h * w
    S, Q = 255 * n, 255 * 255 * n
    assert Q < 2 ** 63 and n * Q > 2 ** 63                                          # the sums fit int64; N Q does not, and need not
    parts = -(-h // 256) * w                                                        # pixels of one part of fdn_pair_moments_u8
    assert 255 * 255 * parts < 2 ** 63
    half = [S // 2] * 3 + [Q // 4 + 7 * n] * 3                                      # a restored image of mean 127.5 and variance 7
    flat_gt = [S] * 3 + [Q] * 3 + half + [255]
    rows = correct.correction_coefficients([flat_gt], "mean_var", n=n)[0]
    assert rows[0][:3] == [127.5, 0.0, 255.0] and rows[0][3:] == [-math.inf, math.inf]
    assert correct.correction_coefficients([flat_gt], "gt_mean", n=n)[0] == [[0.0, 2.0, 0.0, 0.0, 255.0]] * 3
    noisy_gt = [S // 2] * 3 + [Q // 4 + 28 * n] * 3 + half + [255]
    assert correct.correction_coefficients([noisy_gt], "mean_var", n=n)[0][1][1] == 2.0


def test_degenerate_images_give_nan_for_that_image_only():
    gt, rs = ref.textured(20, 30, seed=3, n=3)
    flat = rs.copy()
    flat[1, :, :, 2] = 77                                                           # a flat channel of image 1
    got = correct.correction_coefficients([ref.moments(a, b) for a, b in zip(gt, flat)], "mean_var", n=600)
    assert got[0] == ref.coefficients(gt[0], flat[0], "mean_var") and got[2] == ref.coefficients(gt[2], flat[2], "mean_var")
    assert all(math.isfinite(v) for v in got[1][0][:3] + got[1][1][:3]) and math.isnan(got[1][2][1]) and got[1][2][0] == 77.0
    assert all(same(g, x) for gr, wr in zip(got[1], ref.coefficients(gt[1], flat[1], "mean_var")) for g, x in zip(gr, wr))
    assert np.isnan(ref.corrected(gt[1], flat[1], "mean_var")[:, :, 2]).all() and np.isfinite(ref.corrected(gt[1], flat[1], "mean_var")[:, :, :2]).all()
    assert math.isnan(ref.psnr(gt[1], ref.corrected(gt[1], flat[1], "mean_var")))
    black = rs.copy()
    black[1] = 0
    got = correct.correction_coefficients([ref.moments(a, b) for a, b in zip(gt, black)], "gt_mean", n=600)
    assert all(math.isnan(row[1]) for row in got[1]) and all(math.isfinite(row[1]) for k in (0, 2) for row in got[k])
    assert np.isnan(ref.corrected(gt[1], black[1], "gt_mean")).all()
    # a flat restored image is not degenerate for gt_mean
    assert correct.correction_coefficients([ref.moments(gt[1], flat[1])], "gt_mean", n=600) == [ref.coefficients(gt[1], flat[1], "gt_mean")]


CASES = [((6, 7), 0.6, 20.0), ((33, 65), 1.8, -50.0), ((70, 90), 0.7, 20.0), ((256, 256), 1.4, -30.0), ((720, 1280), 0.6, 20.0)]


def test_affine_map_is_the_references_two_passes():
    """scripts/metrics/calculate_psnr_ssim.py:38-54 in float32, corrected twice, against the single affine map in double: the largest PSNR
    difference and the largest |dz| over five textured pairs whose restored / gt standard-deviation ratio lies in [0.5, 2]"""
    worst_p = worst_z = 0.0
    for (h, w), gain, offset in CASES:
        gt, rs = ref.textured(h, w, seed=h * w, gain=gain, offset=offset)
        for c in range(3):
            assert 0.5 <= rs[:, :, c].std() / gt[:, :, c].std() <= 2.0, (h, w, c)
        z, f = ref.corrected(gt, rs, "mean_var"), ref.reference_mean_var_f32(gt, rs)
        assert f.dtype == z.dtype == np.float32
        dz = float(np.abs(z.astype(np.float64) - f.astype(np.float64)).max())
        dp = abs(ref.psnr(gt, z) - ref.psnr(gt, f))
        print(f"{h}x{w} gain {gain}: |dz| max {dz:.3e} codes, |dPSNR| {dp:.3e} dB, z in [{z.min():.1f}, {z.max():.1f}]")
        worst_p, worst_z = max(worst_p, dp), max(worst_z, dz)
        # what the corrected image is: the ground truth's mean and standard deviation, channel by channel
        for c in range(3):
            assert abs(z[:, :, c].astype(np.float64).mean() - gt[:, :, c].mean()) < 1e-5 and abs(z[:, :, c].astype(np.float64).std() - gt[:, :, c].std()) < 1e-5
    print(f"worst |dPSNR| {worst_p:.3e} dB, worst |dz| {worst_z:.3e} codes")
    assert 8 * MEASURED_DPSNR < 1e-4 and 8 * MEASURED_DZ < 1e-2
    assert worst_p <= 8 * MEASURED_DPSNR and worst_z <= 8 * MEASURED_DZ


def test_gpu_inputs_are_well_conditioned():
    """the inputs of tests/test_gpu_correct.py: the truth's z inside [-64, 320], and the oracle's float32 3-D SSIM within a fifth of that
    test's bound (2e-5) of the same map in float64, so that the bound measures the kernel and not the reference's own rounding"""
    import torch
    import fdn_oracle as O
    chw = lambda a: torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))
    gb, rb = ref.gpu_batch()
    pairs = [(s, *ref.gpu_case(s)) for s in ref.GPU_SHAPES] + [((33, 65, 0), a, b) for a, b in zip(gb, rb)]
    for shape, gt, rs in pairs:
        for mode in correct.MODES:
            z = ref.corrected(gt, rs, mode)
            assert np.isfinite(z).all() and z.min() >= -64 and z.max() <= 320, (shape, mode)
            own = abs(O.ssim_3d(chw(gt), chw(z), shape[2]) - ref.ssim_3d_f64(gt, z, shape[2]))
            print(f"{shape} {mode}: the oracle's float32 map against float64 {own:.2e}, z in [{z.min():.1f}, {z.max():.1f}]")
            assert own < 4e-6, (shape, mode, own)


def test_gt_mean_restatement():
    gt, _ = ref.textured(24, 31, seed=9)
    half = gt // 2
    (_, s, _, lo, hi), = {tuple(r) for r in ref.coefficients(gt, half, "gt_mean")}
    assert 1.98 < s < 2.05 and (lo, hi) == (0.0, 255.0)
    z = ref.corrected(gt, half, "gt_mean")
    assert z.min() >= 0 and z.max() <= 255 and ref.psnr(gt, z) > ref.psnr(gt, half.astype(np.float32)) + 20
    assert np.array_equal(ref.corrected(gt, gt, "gt_mean"), gt.astype(np.float32)) and ref.psnr(gt, ref.corrected(gt, gt, "mean_var")) == math.inf


@pytest.fixture(scope="module")
def clis():
    sys.path.insert(0, PKG)
    import calculate_psnr_ssim
    import validate_fdn
    return calculate_psnr_ssim, validate_fdn


def _folders(tmp_path):
    from PIL import Image
    g = np.random.default_rng(0)
    gt, rs = tmp_path / "gt", tmp_path / "rs"
    gt.mkdir(); rs.mkdir()
    for n in "ab":
        Image.fromarray(g.integers(0, 256, (16, 20, 3), dtype=np.uint8)).save(gt / f"{n}.png")
        Image.fromarray(g.integers(0, 256, (16, 20, 3), dtype=np.uint8)).save(rs / f"{n}.png")
    return gt, rs


def test_command_lines_parse_the_correction(clis, tmp_path, capsys):
    score, validate = clis
    gt, rs = _folders(tmp_path)
    base = ["--gt", str(gt / "*.png"), "--restored", str(rs / "*.png")]
    for mode in ("gt_mean", "mean_var"):
        assert score.parse_args(base + ["--correct", mode]).correct == mode
    assert score.parse_args(base).correct is None
    for argv in (base + ["--correct", "mean"], base + ["--correct"], base + ["--correct_mean_var"], base + ["--correct", "mean_var", "--correct_mean_var"]):
        with pytest.raises(SystemExit):
            score.parse_args(argv)
    assert "--correct mean_var" in capsys.readouterr().err                          # the refusal says what to use instead
    vbase = ["--fdn", "unused.pth", "--lq", str(rs / "*.png"), "--gt", str(gt / "*.png")]
    assert validate.parse_args(vbase + ["--correct", "gt_mean"]).correct == "gt_mean"
    assert not hasattr(validate.parse_args(vbase), "correct")                       # absent unless given, as --lowlight
    for argv in (vbase + ["--correct", "both"], vbase + ["--correct"]):
        with pytest.raises(SystemExit):
            validate.parse_args(argv)
    assert validate.csv_header(validate.parse_args(vbase)) == "frame,psnr,ssim,ratio"
    assert validate.csv_header(validate.parse_args(vbase + ["--correct", "mean_var"])) == "frame,psnr,ssim,ratio,psnr_corr,ssim_corr"
    assert validate.csv_header(validate.parse_args(vbase + ["--lowlight", "--correct", "gt_mean"])) == "frame,psnr,ssim,ratio,loe,deltae,psnr_corr,ssim_corr"
