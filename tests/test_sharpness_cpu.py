"""CPU: the deblurring evaluation's definitions and host side.  The numpy restatement of tests/sharpness_ref.py is held to a dense-matrix
evaluation of G, U, G (the edge residual N), to the reference's own EdgeLoss recorded in tests/golden/sharpness.npz, and to a
scipy.signal.convolve2d transcription of the GMSD authors' MATLAB code; the entry points of include/fdn_sharpness.h in libfdn_sharpness.so
are checked for their version, their generated prototype table, fdn_gmsd_dims and every argument refusal before any launch; and the
command lines for their argument errors.  No GPU compute."""
import ctypes
import importlib.util
import math
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as entry  # noqa: F401  (puts the package on sys.path)
import sharpness_ref as ref
from fdn_hip import sharpness  # noqa: E402  (the module under test: without it nothing here has a subject)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fdn-tip2025_amd")
NAMES = ["fdn_sharpness_abi_version", "fdn_edge_ws", "fdn_edge_u8", "fdn_gmsd_dims", "fdn_gmsd_ws", "fdn_gmsd_u8"]
GOLDEN_SIZES = [(1, 1), (2, 3), (5, 5), (6, 7), (7, 6), (33, 47), (64, 90)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(sharpness.lib_path()):
        entry.build()
    return sharpness.lib()


def gauss_matrix(n):
    """20 G as an n x n integer matrix: row p holds the weights k of the clamped coordinates p - 2 .. p + 2 (replicate padding)"""
    m = np.zeros((n, n), dtype=np.int64)
    for p in range(n):
        for i, k in zip(range(-2, 3), (1, 5, 8, 5, 1)):
            m[p, min(max(p + i, 0), n - 1)] += k
    return m


@pytest.mark.parametrize("h", range(1, 6))
@pytest.mark.parametrize("w", range(1, 6))
def test_residual_is_dense_g_u_g(h, w):
    """N = 160000 d - 400 G(U(400 G(d))) with G a matrix product per axis and U a mask: every border case of 1 .. 5 rows and columns"""
    g = np.random.default_rng(h * 10 + w)
    a, b = g.integers(0, 256, (h, w, 3), dtype=np.uint8), g.integers(0, 256, (h, w, 3), dtype=np.uint8)
    gh, gw = gauss_matrix(h), gauss_matrix(w)
    mask = np.zeros((h, w), dtype=np.int64)
    mask[::2, ::2] = 4
    want = np.empty((h, w, 3), dtype=np.int64)
    for c in range(3):
        d = a[:, :, c].astype(np.int64) - b[:, :, c].astype(np.int64)
        want[:, :, c] = 160000 * d - gh @ (mask * (gh @ d @ gw.T)) @ gw.T
    got = ref.edge_residual(a, b)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert np.abs(got).max() <= 204000000 < 2 ** 31                                     # int32 holds it
    assert not ref.edge_residual(a, a).any() and ref.edge_error(a, a) == 0.001          # sqrt(1e-6) per element


def test_residual_bound_is_reached_by_no_image():
    """|N| <= 160000 * 255 + 400 * 4 * 400 * 255 whatever the image: the weights of each pass sum to 400"""
    assert 160000 * 255 + 400 * 4 * 400 * 255 == 204000000
    for n in range(1, 9):
        assert (gauss_matrix(n).sum(axis=1) == 20).all()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "sharpness.npz"))


def test_edge_error_is_the_references_edge_loss(golden):
    """the restatement's figure against the reference's formula in float64, as tests/golden/make_golden_sharpness.py recorded it.  The
    bound is 8 times the fixture's own largest |float32 - float64| of the reference (a float32 pipeline of about ten chained operations
    held against float64), read from the file."""
    gap = float(golden["gap"])
    assert 0 < gap < 1e-6
    n = len([k for k in golden.files if k.startswith("a_")])
    assert n == 2 * len(GOLDEN_SIZES)
    worst64 = worst32 = 0.0
    for k in range(n):
        a, b = golden[f"a_{k}"], golden[f"b_{k}"]
        assert a.dtype == b.dtype == np.uint8 and a.shape == b.shape == GOLDEN_SIZES[k // 2] + (3,)
        got = ref.edge_error(a, b)
        d64, d32 = abs(got - float(golden[f"f64_{k}"])), abs(got - float(golden[f"f32_{k}"]))
        print(f"{a.shape[0]}x{a.shape[1]} pair {k % 2}: {got:.9e}, from the reference's float64 {d64:.2e}, from its float32 {d32:.2e}")
        worst64, worst32 = max(worst64, d64), max(worst32, d32)
        assert abs(float(golden[f"f32_{k}"]) - float(golden[f"f64_{k}"])) <= gap
    print(f"worst distance to the reference's float64 {worst64:.2e}, to its float32 {worst32:.2e}; bound 8 x {gap:.2e}")
    assert worst64 <= 8 * gap
    assert worst32 <= 9 * gap                                                           # the triangle inequality, not a second bound


def matlab_gmsd(a, b, bgr=True):
    """GMSD.m of Xue, Zhang, Mou and Bovik, line by line, on the luma 0.299 R + 0.587 G + 0.114 B in [0, 255].  MATLAB's
    conv2(., ., 'same') keeps the part of the full convolution that starts at ceil((k - 1) / 2): for the 2 x 2 average that is row and
    column 1 of 'full' (scipy's mode='same' starts at 0 for an even kernel, so the slice is written out); for 3 x 3 the two agree."""
    from scipy.signal import convolve2d
    T, down = 170.0, 2
    dx = np.array([[1, 0, -1], [1, 0, -1], [1, 0, -1]], dtype=np.float64) / 3
    dy = dx.T
    ave = np.ones((2, 2)) / 4
    maps = []
    for img in (a, b):
        y = ref.gray1000(img, bgr).astype(np.float64) / 1000
        h, w = y.shape
        y = convolve2d(y, ave, mode="full")[1:h + 1, 1:w + 1][::down, ::down]
        maps.append(np.sqrt(convolve2d(y, dx, mode="same") ** 2 + convolve2d(y, dy, mode="same") ** 2))
    g1, g2 = maps
    q = (2 * g1 * g2 + T) / (g1 ** 2 + g2 ** 2 + T)
    return float(np.std(q, ddof=1)), q, g1, g2


@pytest.mark.parametrize("shape", [(1, 3), (3, 1), (2, 4), (3, 5), (6, 7), (7, 6), (33, 47), (64, 90), (120, 161)])
def test_gmsd_is_the_authors_matlab(shape):
    for k, (a, b) in enumerate((ref.soft_pair(*shape, seed=7), ref.random_pair(*shape, seed=8))):
        want, q, g1, g2 = matlab_gmsd(a, b)
        got = ref.gmsd(a, b)
        print(f"{shape} pair {k}: GMSD {got!r}, MATLAB transcription {want!r}, diff {got - want:+.1e}")
        assert abs(got - want) <= 1e-13
        assert np.abs(ref.gms_map(a, b) - q).max() <= 1e-13
        assert np.abs(ref.gradient_terms(a) - g1).max() <= 1e-10 and np.abs(ref.gradient_terms(b) - g2).max() <= 1e-10   # of values up to 360
        assert q.shape == ref.gmsd_dims(*shape)
    a, b = ref.random_pair(*shape, seed=9)
    flip = lambda x: np.ascontiguousarray(x[:, :, ::-1])
    assert ref.gmsd(flip(a), flip(b), bgr=False) == ref.gmsd(a, b) and np.array_equal(ref.grad2(flip(a), bgr=False), ref.grad2(a))
    assert (ref.gms_map(a, a) == 1.0).all() and ref.gmsd(a, a) == 0.0                    # sqrt(fl(A^2)) == A
    assert ref.grad2(a).max() < 2 ** 45


def test_soft_pairs_are_soft():
    """what the figures are for: the blurred copy has the smaller mean gradient, and scores worse than the image against itself"""
    a, b = ref.soft_pair(64, 90, seed=3)
    assert ref.mean_gradient(b) < ref.mean_gradient(a)                                  # a ratio below 1: softer than the truth
    assert ref.gmsd(a, b) > ref.gmsd(a, a) == 0.0 and ref.edge_error(a, b) > ref.edge_error(a, a) == 0.001


def test_version_and_generated_table(lib, monkeypatch):
    spec = importlib.util.spec_from_file_location("gen_abi_table", os.path.join(ROOT, "tools", "gen_abi_table.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    from fdn_hip import _abi_sharpness as table
    protos, names, members, versions = gen.build_table(headers=["fdn_sharpness.h"])
    assert table.PROTOTYPES == protos and table.ARG_NAMES == names and list(protos) == members["fdn_sharpness.h"] == NAMES
    assert table.VERSION == versions["fdn_sharpness.h"] == ("fdn_sharpness_abi_version", 1)
    assert "fdn_sharpness.h" not in gen.HEADERS                                    # the one table of libfdn_hip.so stays what it was
    assert lib.fdn_sharpness_abi_version() == 1 == sharpness.ABI_VERSION
    assert lib.fdn_edge_ws.restype == lib.fdn_gmsd_ws.restype == ctypes.c_long
    assert lib.fdn_edge_u8.argtypes == [ctypes.c_void_p] * 2 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 4
    assert lib.fdn_gmsd_u8.argtypes == [ctypes.c_void_p] * 2 + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 5
    assert table.ARG_NAMES["fdn_gmsd_u8"] == ["a", "b", "B", "h", "w", "bgr", "grad2", "map", "ws", "out", "stream"]
    header = open(os.path.join(ROOT, "include", "fdn_sharpness.h")).read()
    assert f"FDN_EDGE_TILE = {sharpness.EDGE_TILE}, FDN_GMSD_TILE = {sharpness.GMSD_TILE}" in header
    # neither of the other libraries holds these entry points
    import fdn_hip
    from fdn_hip import correct
    assert not hasattr(fdn_hip.lib(), "fdn_gmsd_u8") and not hasattr(correct.lib(), "fdn_gmsd_u8")
    # a library of another version is refused with the sentence of fdn_hip.lib()
    monkeypatch.setattr(sharpness, "_lib", None)
    monkeypatch.setattr(sharpness, "ABI_VERSION", 2)
    with pytest.raises(ImportError, match=r"libfdn_sharpness\.so has sharpness ABI version 1, this binding needs 2: rebuild with build\.sh"):
        sharpness.lib()
    assert sharpness._lib is None


def test_gmsd_dims_rule(lib):
    for h, w in [(1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (64, 90), (65, 91), (720, 1280), (1, 2 ** 31 - 1), (46340, 46340)]:
        assert sharpness.gmsd_dims(h, w) == ref.gmsd_dims(h, w) == ((h + 1) // 2, (w + 1) // 2)
    hd, wd = ctypes.c_int(-7), ctypes.c_int(-7)
    for h, w in [(0, 4), (4, 0), (-1, 4), (4, -2), (46341, 46341), (2, 2 ** 30)]:
        assert lib.fdn_gmsd_dims(h, w, ctypes.byref(hd), ctypes.byref(wd)) == 1 and (hd.value, wd.value) == (-7, -7)
    assert lib.fdn_gmsd_dims(4, 4, None, ctypes.byref(wd)) == 1 and lib.fdn_gmsd_dims(4, 4, ctypes.byref(hd), None) == 1
    from fdn_hip import FdnHipError
    with pytest.raises(FdnHipError, match="fdn_gmsd_dims"):
        sharpness.gmsd_dims(0, 3)


GOOD = dict(B=2, h=40, w=50)
BAD = [dict(B=0), dict(B=-1), dict(h=0), dict(h=-4), dict(w=0), dict(w=-1), dict(h=46341, w=46341), dict(h=2 ** 31 - 1, w=2)]
ONE_POINT = [dict(h=1, w=1), dict(h=2, w=2), dict(h=1, w=2), dict(h=2, w=1), dict(B=1, h=2, w=2)]     # n = hd wd < 2: no standard deviation


def check_argument_errors(lib):
    """every refusal of include/fdn_sharpness.h returns its code before any launch: FDN_ERR_ARG = 1, FDN_ERR_UNSUPPORTED = 4 (the
    pointers are never dereferenced, and a machine without a GPU has nothing to launch on); the workspace queries answer 0 to the same
    sizes"""
    p = ctypes.c_void_p(64)                                                        # never dereferenced

    def edge(ptrs=None, **kw):
        a = {**GOOD, **kw}
        q = dict(a=p, b=p, resid=None, ws=p, out=p)
        q.update(ptrs or {})
        return lib.fdn_edge_u8(q["a"], q["b"], a["B"], a["h"], a["w"], q["resid"], q["ws"], q["out"], None)

    def gmsd(ptrs=None, bgr=1, **kw):
        a = {**GOOD, **kw}
        q = dict(a=p, b=p, grad2=None, map=None, ws=p, out=p)
        q.update(ptrs or {})
        return lib.fdn_gmsd_u8(q["a"], q["b"], a["B"], a["h"], a["w"], bgr, q["grad2"], q["map"], q["ws"], q["out"], None)

    for bad in BAD:
        assert edge(**bad) == 1 and gmsd(**bad) == 1, bad
        a = {**GOOD, **bad}
        assert lib.fdn_edge_ws(a["B"], a["h"], a["w"]) == 0 and lib.fdn_gmsd_ws(a["B"], a["h"], a["w"]) == 0, bad
    for bad in ONE_POINT:
        a = {**GOOD, **bad}
        assert gmsd(**bad) == 1 and lib.fdn_gmsd_ws(a["B"], a["h"], a["w"]) == 0, bad
        assert lib.fdn_edge_ws(a["B"], a["h"], a["w"]) == a["B"], bad            # the edge error of one pixel is defined
    for k in ("a", "b", "ws", "out"):
        assert edge({k: None}) == 1 and gmsd({k: None}) == 1, k
    for off in (1, 2, 4, 68):                                                       # ws not 8-byte aligned
        assert edge({"ws": ctypes.c_void_p(64 + off)}) == 1 and gmsd({"ws": ctypes.c_void_p(64 + off)}) == 1, off
    # more workgroups than a grid holds: 2 tiles per image and 2^30 images
    assert edge(B=2 ** 30, h=33, w=1) == 4 and gmsd(B=2 ** 30, h=1, w=130) == 4
    assert lib.fdn_edge_ws(2, 40, 50) == 2 * 2 * 2 and lib.fdn_gmsd_ws(2, 40, 50) == 4 * 2 * 1 * 1
    assert lib.fdn_edge_ws(1, 720, 1280) == 23 * 40 and lib.fdn_gmsd_ws(1, 720, 1280) == 4 * 12 * 20
    assert lib.fdn_edge_ws(3, 32, 33) == 3 * 2 and lib.fdn_gmsd_ws(3, 64, 66) == 4 * 3 * 2


def test_entry_points_validate_arguments_without_gpu(lib):
    check_argument_errors(lib)


def test_module_refuses_without_a_device():
    from fdn_hip import FdnHipError
    z = np.zeros((8, 8, 3), np.uint8)
    for f in (sharpness.edge_error_u8, sharpness.edge_residual_u8, sharpness.gmsd_u8, sharpness.gmsd_map_u8, sharpness.sharpness_metrics):
        with pytest.raises(FdnHipError, match="Image shapes are different"):
            f(z, np.zeros((8, 9, 3), np.uint8))
        with pytest.raises(FdnHipError, match="takes uint8 images"):
            f(z.astype(np.float32), z.astype(np.float32))
    with pytest.raises(FdnHipError, match="mean_gradient_u8 takes uint8 images"):
        sharpness.mean_gradient_u8(z.astype(np.float32))
    assert sharpness.gmsd_from_sums(6.0, 6.0, 6) == 0.0 and sharpness.gmsd_from_sums(3.0, 5.0, 2) == math.sqrt(0.5)
    assert sharpness.gmsd_from_sums(3.0, 3.0 - 1e-15, 3) == 0.0                         # a rounding below zero is zero
    src = open(os.path.join(PKG, "fdn_hip", "sharpness.py")).read()
    assert "oracle" not in src and "tests" not in src.replace("tests/", "")           # the product path stands without the yardsticks


@pytest.fixture(scope="module")
def clis():
    sys.path.insert(0, PKG)
    import calculate_sharpness_metrics
    import validate_fdn
    return calculate_sharpness_metrics, validate_fdn


def test_command_lines_parse_their_arguments(clis, tmp_path, capsys):
    from PIL import Image
    score, validate = clis
    g = np.random.default_rng(0)
    gt, rs = tmp_path / "gt", tmp_path / "rs"
    gt.mkdir(); rs.mkdir()
    for n in "ab":
        Image.fromarray(g.integers(0, 256, (16, 20, 3), dtype=np.uint8)).save(gt / f"{n}.png")
        Image.fromarray(g.integers(0, 256, (16, 20, 3), dtype=np.uint8)).save(rs / f"{n}.png")
    Image.fromarray(g.integers(0, 256, (16, 20, 3), dtype=np.uint8)).save(rs / "c.png")
    base = ["--restored", str(rs / "[ab].png")]
    a = score.parse_args(base + ["--gt", str(gt / "*.png")])
    assert [tuple(os.path.basename(p) for p in it) for it in a.items] == [("a.png", "a.png"), ("b.png", "b.png")] and a.batch == 8
    assert [len(it) for it in score.parse_args(base).items] == [1, 1]                # without --gt: the restored images alone
    for argv in (["--gt", str(gt / "*.png")],                                        # --restored is required
                 base + ["--batch", "0"],
                 base + ["--save-gms-map", str(tmp_path / "maps")],                  # a map is of a pair
                 ["--restored", str(rs / "*.png"), "--gt", str(gt / "*.png")],       # 3 restored, 2 ground truths
                 ["--restored", str(rs / "*.jpg")],
                 base + ["--gt", str(gt / "*.jpg")]):
        with pytest.raises(SystemExit):
            score.parse_args(argv)
    capsys.readouterr()
    assert score.sharpness_line({"edge": 0.5, "gmsd": 0.25, "grad_ratio": 2.0}) == "edge: 0.500000, GMSD: 0.250000, grad ratio: 2.000000"
    assert score.map_bytes(np.array([[0.0, 0.5, 1.0, 1.0 + 1e-7]], np.float32)).tolist() == [[0, 128, 255, 255]]
    vbase = ["--fdn", "unused.pth", "--lq", str(rs / "[ab].png"), "--gt", str(gt / "*.png")]
    assert validate.parse_args(vbase + ["--sharpness"]).sharpness is True
    assert not hasattr(validate.parse_args(vbase), "sharpness")                      # absent unless given, as --lowlight
    with pytest.raises(SystemExit):
        validate.parse_args(vbase + ["--sharpness", "yes"])
    assert validate.csv_header(validate.parse_args(vbase)) == "frame,psnr,ssim,ratio"
    assert validate.csv_header(validate.parse_args(vbase + ["--sharpness"])) == "frame,psnr,ssim,ratio,edge,gmsd,grad_ratio"
    assert validate.csv_header(validate.parse_args(vbase + ["--sharpness", "--lowlight", "--correct", "gt_mean"])) == \
        "frame,psnr,ssim,ratio,loe,deltae,psnr_corr,ssim_corr,edge,gmsd,grad_ratio"
