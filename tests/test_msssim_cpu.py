"""CPU: multi-scale SSIM's definitions and host side.  The numpy restatement of tests/msssim_ref.py is held to an independent statement
of the pyramid (pad by replication to even sizes, then block-sum) and, pixel by pixel, to a truth that shares neither its order nor its
precision (the direct 121-tap sum in np.longdouble); the entry points of include/fdn_msssim.h in libfdn_msssim.so are checked for their
version, their generated prototype table, fdn_msssim_dims and every argument refusal before any launch; the host step for its exact
cases; and the three command lines for their arguments.  No GPU compute.

The bound of (c), derived and not tuned.  U = 2^-53.  A windowed moment is a sum of non-negative terms g_i g_j x formed in two passes of
11 products and 11 additions each (the first addition, to 0, is exact): at most 12 roundings per pass, so |dm| <= 24 U m to first order.
    va = m_aa - m_a^2:  |d va| <= 24 U m_aa + (2 * 24 + 1) U m_a^2 + U |va|   (the product m_a * m_a rounds once, the difference once)
    vb likewise; vab = m_ab - m_a m_b with m_ab <= (m_aa + m_bb) / 2 and m_a m_b <= (m_a^2 + m_b^2) / 2 is bounded by the mean of the two.
With S = m_aa + m_bb + m_a^2 + m_b^2 + C2' and D = va + vb + C2' >= C2' > 0, the numerator N = 2 vab + C2' has |dN| <= about 50 U S and
the denominator |dD| <= about 50 U S, |N| <= D, and the quotient rounds once more:
    |d cs| <= (|dN| + |cs| |dD|) / D + U |cs| <= about 107 U S / D;   K = 128 is used.
l = (2 m_a m_b + C1') / (m_a^2 + m_b^2 + C1') has no cancellation (every term is non-negative): |dl| <= about 100 U l <= K U, and
ss = l cs with l <= 1:  |d ss| <= |d cs| + |cs| |dl| + U <= K U (S / D + 1).
The right-hand sides are evaluated from the truth's values.  The ratio S / D reaches about 1e3 on bright flat regions (S about 4 L^2 q^2
over D about C2' = 9e-4 L^2 q^2), which is why a flat tolerance would be wrong."""
import ctypes
import importlib.util
import math
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as entry  # noqa: F401  (puts the package on sys.path)
import msssim_ref as ref
from fdn_hip import msssim  # noqa: E402  (the module under test: without it nothing here has a subject)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fdn-tip2025_amd")
NAMES = ["fdn_msssim_abi_version", "fdn_msssim_dims", "fdn_msssim_ws", "fdn_msssim_u8", "fdn_msssim_luma"]
SHAPES = [(161, 161), (161, 200), (193, 177), (176, 208)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(msssim.lib_path()):
        entry.build()
    return msssim.lib()


# ---- (a) the table and the header -----------------------------------------------------------------------------------------------------
def test_version_and_generated_table(lib, monkeypatch):
    spec = importlib.util.spec_from_file_location("gen_abi_table", os.path.join(ROOT, "tools", "gen_abi_table.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    from fdn_hip import _abi_msssim as table
    protos, names, members, versions = gen.build_table(headers=["fdn_msssim.h"])
    assert table.PROTOTYPES == protos and table.ARG_NAMES == names and list(protos) == members["fdn_msssim.h"] == NAMES
    assert table.VERSION == versions["fdn_msssim.h"] == ("fdn_msssim_abi_version", 1)
    assert "fdn_msssim.h" not in gen.HEADERS                                       # the one table of libfdn_hip.so stays what it was
    assert lib.fdn_msssim_abi_version() == 1 == msssim.ABI_VERSION
    assert lib.fdn_msssim_ws.restype == ctypes.c_long
    assert lib.fdn_msssim_u8.argtypes == [ctypes.c_void_p] * 2 + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 8
    assert lib.fdn_msssim_luma.argtypes == [ctypes.c_void_p] * 2 + [ctypes.c_int] * 4 + [ctypes.c_long] + [ctypes.c_void_p] * 8
    assert table.ARG_NAMES["fdn_msssim_u8"] == ["a", "b", "B", "h", "w", "mode", "bgr", "taps11", "pyr_a", "pyr_b", "cs_map", "ss_map", "ws", "out",
                                                "stream"]
    assert table.ARG_NAMES["fdn_msssim_luma"] == ["a", "b", "B", "h", "w", "bits", "stride", "taps11", "pyr_a", "pyr_b", "cs_map", "ss_map", "ws",
                                                  "out", "stream"]
    header = open(os.path.join(ROOT, "include", "fdn_msssim.h")).read()
    assert (f"FDN_MSSSIM_LEVELS = {msssim.LEVELS}, FDN_MSSSIM_MIN_SIDE = {msssim.MIN_SIDE}, FDN_MSSSIM_TILE_H = {msssim.TILE_H}, "
            f"FDN_MSSSIM_TILE_W = {msssim.TILE_W}") in header
    assert f"FDN_MSSSIM_RGB = {msssim.MODES['rgb']}, FDN_MSSSIM_GRAY = {msssim.MODES['gray']}" in header
    assert (msssim.LEVELS, msssim.MIN_SIDE, msssim.WEIGHTS) == (ref.LEVELS, ref.MIN_SIDE, ref.WEIGHTS) and abs(sum(ref.WEIGHTS) - 1.0001) < 1e-12
    assert np.array_equal(msssim._TAPS, ref.taps()) and msssim._TAPS.dtype == np.float64      # the window the host hands over
    # none of the other libraries holds these entry points
    import fdn_hip
    from fdn_hip import correct, sharpness
    for other in (fdn_hip.lib(), correct.lib(), sharpness.lib()):
        assert not hasattr(other, "fdn_msssim_u8")
    # a library of another version is refused with the sentence of fdn_hip.lib()
    monkeypatch.setattr(msssim, "_lib", None)
    monkeypatch.setattr(msssim, "ABI_VERSION", 2)
    with pytest.raises(ImportError, match=r"libfdn_msssim\.so has msssim ABI version 1, this binding needs 2: rebuild with build\.sh"):
        msssim.lib()
    assert msssim._lib is None


def test_dims_rule(lib):
    for h, w in SHAPES + [(171, 171), (720, 1280), (1080, 1920), (161, 2 ** 31 // 161 - 1), (46340, 46340)]:
        assert msssim.msssim_dims(h, w) == ref.dims(h, w)
    assert msssim.msssim_dims(161, 161) == ([(161, 161), (81, 81), (41, 41), (21, 21), (11, 11)], [(151, 151), (71, 71), (31, 31), (11, 11), (1, 1)])
    assert msssim.msssim_dims(193, 177)[0] == [(193, 177), (97, 89), (49, 45), (25, 23), (13, 12)]         # odd at every level
    arr = [(ctypes.c_int * 5)(*[-7] * 5) for _ in range(4)]
    for h, w in [(160, 161), (161, 160), (0, 500), (500, -1), (46341, 46341), (161, 2 ** 31 // 161 + 1)]:
        assert lib.fdn_msssim_dims(h, w, *arr) == 1 and all(list(a) == [-7] * 5 for a in arr), (h, w)
    for k in range(4):
        assert lib.fdn_msssim_dims(200, 200, *[None if i == k else arr[i] for i in range(4)]) == 1
    from fdn_hip import FdnHipError
    with pytest.raises(FdnHipError, match="at least 161x161"):
        msssim.msssim_dims(160, 400)


GOOD = dict(B=2, h=170, w=200)
BAD = [dict(B=0), dict(B=-1), dict(h=160), dict(w=160), dict(h=0), dict(w=-3), dict(h=46341, w=46341), dict(h=2 ** 31 - 1, w=161)]


def check_argument_errors(lib):
    """every refusal of include/fdn_msssim.h returns its code before any launch: FDN_ERR_ARG = 1, FDN_ERR_UNSUPPORTED = 4 (the pointers
    are never dereferenced - taps11 is read only after the checks - and a machine without a GPU has nothing to launch on); the workspace
    query answers 0 to the same sizes"""
    p = ctypes.c_void_p(64)                                                        # never dereferenced

    def u8(ptrs=None, mode=0, bgr=1, **kw):
        a = {**GOOD, **kw}
        q = dict(a=p, b=p, taps=p, pyr_a=None, pyr_b=None, cs=None, ss=None, ws=p, out=p)
        q.update(ptrs or {})
        return lib.fdn_msssim_u8(q["a"], q["b"], a["B"], a["h"], a["w"], mode, bgr, q["taps"], q["pyr_a"], q["pyr_b"], q["cs"], q["ss"], q["ws"],
                                 q["out"], None)

    def luma(ptrs=None, bits=8, stride=None, **kw):
        a = {**GOOD, **kw}
        q = dict(a=p, b=p, taps=p, pyr_a=None, pyr_b=None, cs=None, ss=None, ws=p, out=p)
        q.update(ptrs or {})
        stride = a["h"] * a["w"] * 3 // 2 if stride is None else stride
        return lib.fdn_msssim_luma(q["a"], q["b"], a["B"], a["h"], a["w"], bits, stride, q["taps"], q["pyr_a"], q["pyr_b"], q["cs"], q["ss"],
                                   q["ws"], q["out"], None)

    for bad in BAD:
        assert u8(**bad) == 1 and u8(mode=1, **bad) == 1 and luma(**bad) == 1 and luma(bits=10, **bad) == 1, bad
        a = {**GOOD, **bad}
        assert lib.fdn_msssim_ws(a["B"], 1, a["h"], a["w"]) == 0 and lib.fdn_msssim_ws(a["B"], 3, a["h"], a["w"]) == 0, bad
    for planes in (0, 2, 4, -1):
        assert lib.fdn_msssim_ws(2, planes, 170, 200) == 0
    for k in ("a", "b", "taps", "ws", "out"):
        assert u8({k: None}) == 1 and luma({k: None}) == 1, k
    for off in (1, 2, 4, 68):                                                       # ws not 8-byte aligned
        assert u8({"ws": ctypes.c_void_p(64 + off)}) == 1 and luma({"ws": ctypes.c_void_p(64 + off)}) == 1, off
    for mode in (-1, 2, 3):
        assert u8(mode=mode) == 1
    for bits in (0, 9, 12, 16):
        assert luma(bits=bits) == 1
    assert luma(stride=170 * 200 - 1) == 1                                          # frames that overlap their Y planes
    # more workgroups than a grid holds: level 0 of 161 x 161 has 10 x 5 tiles, and 2^30 images
    assert u8(B=2 ** 30, h=161, w=161) == 4 and u8(B=2 ** 30, h=161, w=161, mode=1) == 4 and luma(B=2 ** 30, h=161, w=161) == 4
    # the workspace: two doubles per tile of every plane's five maps (16 x 32 positions a tile), then two int32 pyramids of levels 1 .. 4
    T = lambda mh, mw: -(-mh // msssim.TILE_H) * -(-mw // msssim.TILE_W)      # noqa: E731
    for B, planes, h, w in [(1, 1, 161, 161), (2, 3, 170, 200), (3, 1, 193, 177), (1, 1, 720, 1280)]:
        levels, maps = ref.dims(h, w)
        P = B * planes
        want = 2 * P * sum(T(*m) for m in maps) + (2 * P * sum(a * b for a, b in levels[1:]) + 1) // 2
        assert lib.fdn_msssim_ws(B, planes, h, w) == want, (B, planes, h, w)
    assert lib.fdn_msssim_ws(1, 1, 161, 161) == 2 * (50 + 15 + 2 + 1 + 1) + (2 * (81 * 81 + 41 * 41 + 21 * 21 + 11 * 11) + 1) // 2


def test_entry_points_validate_arguments_without_gpu(lib):
    check_argument_errors(lib)


def test_module_refuses_without_a_device():
    from fdn_hip import FdnHipError
    z = np.zeros((170, 170, 3), np.uint8)
    for f in (msssim.ms_ssim_u8, msssim.ms_ssim_sums_u8, msssim.ms_ssim_pyramids_u8, msssim.ms_ssim_maps_u8):
        with pytest.raises(FdnHipError, match="Image shapes are different"):
            f(z, np.zeros((170, 171, 3), np.uint8))
        with pytest.raises(FdnHipError, match="takes uint8 images"):
            f(z.astype(np.float32), z.astype(np.float32))
        with pytest.raises(FdnHipError, match="rgb or gray"):
            f(z, z, mode="ycbcr")
    from fdn_hip.harness import VideoFormat
    with pytest.raises(ValueError, match="at least 161x161, got 208x160"):
        msssim.MsSsimScore(160, 208, VideoFormat("yuv420p"))
    assert math.isnan(msssim.MsSsimScore(176, 208, VideoFormat("yuv420p")).summary()["ms_ssim_y"])
    src = open(os.path.join(PKG, "fdn_hip", "msssim.py")).read()
    assert "oracle" not in src and "tests" not in src.replace("tests/", "")           # the product path stands without the yardsticks


# ---- (b) the pyramid ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (2, 1), (3, 3), (4, 6), (5, 8), (7, 7), (12, 13), (161, 161), (193, 177), (176, 208)])
def test_pyramid_is_replicate_pad_and_block_sum(shape):
    """the rule (an index equal to the size is taken at size - 1) against: pad by replication to even sizes, then sum 2 x 2 blocks -
    imfilter(., ones(2) / 4, 'symmetric', 'same') followed by (1:2:end, 1:2:end), times 4"""
    h, w = shape
    x = np.random.default_rng(h * 1000 + w).integers(0, 255001, (h, w), dtype=np.int64)
    p = np.pad(x, ((0, h % 2), (0, w % 2)), mode="edge")
    want = p.reshape(p.shape[0] // 2, 2, p.shape[1] // 2, 2).sum(axis=(1, 3))
    got = ref.downsample(x)
    assert got.dtype == np.int64 and got.shape == ((h + 1) // 2, (w + 1) // 2) and np.array_equal(got, want)
    if h % 2 == 0 and w % 2 == 0:                                                      # the 2 x 2 mean of every common implementation
        assert np.array_equal(got, 4 * x.reshape(h // 2, 2, w // 2, 2).mean(axis=(1, 3)))


def test_pyramid_levels_are_exact_int32_with_exact_squares():
    a = np.full((161, 161, 3), 255, np.uint8)
    for mode, q0 in (("rgb", 1), ("gray", 1000)):
        (pl, *_), q, L = ref.planes_u8(a, mode)
        lv = ref.pyramid(pl)
        assert (q, L) == (q0, 255) and [x.shape for x in lv] == ref.dims(161, 161)[0]
        assert all((x == q0 * 255 * 4 ** s).all() for s, x in enumerate(lv))           # q = q0 4^s times the mean
    assert 1000 * 255 * 256 < 2 ** 31 and (1000 * 255 * 256) ** 2 < 2 ** 53
    g = np.random.default_rng(5).integers(0, 256, (20, 24, 3), dtype=np.uint8)
    flip = np.ascontiguousarray(g[..., ::-1])
    for mode in ("rgb", "gray"):
        assert all(np.array_equal(x, y) for x, y in zip(ref.planes_u8(g, mode, bgr=True)[0], ref.planes_u8(flip, mode, bgr=False)[0]))
    assert np.array_equal(ref.planes_u8(g, "rgb", bgr=False)[0][0], g[..., 0]) and np.array_equal(ref.planes_u8(g, "rgb", bgr=True)[0][0], g[..., 2])
    y = np.array([0, 1023, 1024, 65535] * 4, dtype=np.uint16)
    assert ref.plane_luma(np.concatenate([y, y[:8]]), 4, 4, 10)[0].ravel().tolist() == [0, 1023, 1023, 1023] * 4


# ---- (c) the restatement against the truth --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["rgb", "gray"])
@pytest.mark.parametrize("kind", ref.INPUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_restatement_within_the_bound_of_the_truth(shape, kind, mode):
    """pixel by pixel, at every level, for q0 = 1 and 1000 (the first plane of the mode)"""
    a, b = ref.pair(kind, *shape)
    (pa, *_), q0, L = ref.planes_u8(a, mode)
    (pb, *_), _, _ = ref.planes_u8(b, mode)
    res = ref.plane_result(pa, pb, q0, L)
    worst = worst_ratio = 0.0
    for s in range(ref.LEVELS):
        cs, ss, ratio = ref.level_truth(res["pyr_a"][s], res["pyr_b"][s], q0, L, s)
        bc, bs = ref.bound(ratio)
        e_cs, e_ss = np.abs(res["cs"][s] - cs).astype(np.float64), np.abs(res["ss"][s] - ss).astype(np.float64)
        assert cs.shape == res["cs"][s].shape == ref.dims(*shape)[1][s]
        worst = max(worst, float((e_cs / (ref.U * ratio.astype(np.float64))).max()))
        worst_ratio = max(worst_ratio, float(ratio.max()))
        assert (e_cs <= bc).all() and (e_ss <= bs).all(), (s, float((e_cs / bc).max()), float((e_ss / bs).max()))
    print(f"{shape} {kind} {mode}: MS-SSIM {res['ms_ssim']!r}; worst |d cs| = {worst:.2f} U ratio (bound {ref.K_BOUND}), largest ratio {worst_ratio:.3g}")
    if kind == "same":
        assert all((m == 1.0).all() for m in res["cs"] + res["ss"]) and res["ms_ssim"] == 1.0
    if kind == "inverse":
        assert all(m < 0 for m in res["means"]) and res["ms_ssim"] == 0.0
    if kind in ("smooth", "dark", "const"):
        assert 0.99 < res["ms_ssim"] < 1.0
    if kind == "noise":
        assert 0.0 < res["ms_ssim"] < 0.3


# ---- (d) the host step ----------------------------------------------------------------------------------------------------------------
def test_host_step():
    sizes = [151 * 151, 71 * 71, 31 * 31, 11 * 11, 1]
    ones = [(float(n), float(n)) for n in sizes]
    r = msssim.ms_ssim_from_sums(ones, sizes)
    assert r == {"ms_ssim": 1.0, "levels": [1.0] * 5}                                   # equal planes: exactly 1.0
    # a negative mean gives 0.0, and stays on show
    neg = list(ones)
    neg[2] = (-0.25 * sizes[2], 0.5 * sizes[2])
    r = msssim.ms_ssim_from_sums(neg, sizes)
    assert r["ms_ssim"] == 0.0 and r["levels"] == [1.0, 1.0, -0.25, 1.0, 1.0]
    # weights, which of the two sums a level uses, and the order of multiplication
    means = [0.31, 0.52, 0.73, 0.94, 0.85]
    sums = [(m * n, 7.0) for m, n in zip(means[:4], sizes[:4])] + [(7.0, means[4] * sizes[4])]
    r = msssim.ms_ssim_from_sums(sums, sizes)
    lv = [s[1 if i == 4 else 0] / n for i, (s, n) in enumerate(zip(sums, sizes))]
    want = math.pow(lv[0], 0.0448)
    for m, wt in zip(lv[1:], (0.2856, 0.3001, 0.2363, 0.1333)):
        want = want * math.pow(m, wt)
    assert r["levels"] == lv and r["ms_ssim"] == want == ref.from_means(lv)
    assert abs(want - math.exp(sum(wt * math.log(m) for m, wt in zip(means, ref.WEIGHTS)))) < 1e-15
    with pytest.raises(ValueError):
        msssim.ms_ssim_from_sums(ones[:4], sizes)
    # the rgb record: the channels added in the order R, G, B
    rows = [sums, ones, neg]
    rec = msssim._records(rows, 1, 3, sizes)[0]
    per = [msssim.ms_ssim_from_sums(x, sizes) for x in rows]
    assert rec["channels"] == [want, 1.0, 0.0] and rec["ms_ssim"] == (want + 1.0 + 0.0) / 3 and rec["channel_levels"] == [p["levels"] for p in per]
    assert msssim._records(rows, 3, 1, sizes) == per


# ---- (e) the command lines ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clis():
    sys.path.insert(0, PKG)
    import calculate_ms_ssim
    import calculate_video_metrics
    import validate_fdn
    return calculate_ms_ssim, calculate_video_metrics, validate_fdn


def test_command_lines_parse_their_arguments(clis, tmp_path, capsys):
    from PIL import Image
    score, video, validate = clis
    g = np.random.default_rng(0)
    gt, rs = tmp_path / "gt", tmp_path / "rs"
    gt.mkdir(); rs.mkdir()
    for n in "ab":
        Image.fromarray(g.integers(0, 256, (16, 20, 3), dtype=np.uint8)).save(gt / f"{n}.png")
        Image.fromarray(g.integers(0, 256, (16, 20, 3), dtype=np.uint8)).save(rs / f"{n}.png")
    Image.fromarray(g.integers(0, 256, (16, 20, 3), dtype=np.uint8)).save(rs / "c.png")
    base = ["--restored", str(rs / "[ab].png"), "--gt", str(gt / "*.png")]
    a = score.parse_args(base)
    assert [tuple(os.path.basename(p) for p in it) for it in a.items] == [("a.png", "a.png"), ("b.png", "b.png")]
    assert (a.batch, a.mode, a.csv, a.save_map) == (8, "rgb", None, None)
    a = score.parse_args(base + ["--mode", "gray", "--batch", "3", "--csv", "x.csv", "--save-map", "maps"])
    assert (a.batch, a.mode, a.csv, a.save_map) == (3, "gray", "x.csv", "maps")
    for argv in (["--restored", str(rs / "[ab].png")],                              # --gt is required: the score is of a pair
                 ["--gt", str(gt / "*.png")],
                 base + ["--batch", "0"],
                 base + ["--mode", "ycbcr"],
                 ["--restored", str(rs / "*.png"), "--gt", str(gt / "*.png")],       # 3 restored, 2 ground truths
                 ["--restored", str(rs / "*.jpg"), "--gt", str(gt / "*.png")]):
        with pytest.raises(SystemExit):
            score.parse_args(argv)
    assert score.ms_ssim_line({"ms_ssim": 0.5, "levels": [1.0, 0.75, 0.5, 0.25, -0.125]}) == \
        "MS-SSIM: 0.500000 (levels 1.000000 0.750000 0.500000 0.250000 -0.125000)"

    # calculate_video_metrics.py: --ms-ssim is of a pair
    v = video.parse_args(["--ref", "gt.y4m", "out.y4m", "--ms-ssim"])
    assert v.ms_ssim is True and video.parse_args(["--ref", "gt.y4m", "out.y4m"]).ms_ssim is False
    with pytest.raises(SystemExit):
        video.parse_args(["out.y4m", "--ms-ssim"])
    assert "--ms-ssim needs --ref" in capsys.readouterr().err
    assert video.CSV_COLUMNS == ("frame", "psnr_y", "psnr_u", "psnr_v", "psnr_avg", "ssim_y", "mean_y_ref", "mean_y", "cut", "dmean_ref", "dmean")
    assert video.MOTION_COLUMNS == ("mc_psnr", "mc_psnr_ref", "tc_rmse", "moving", "mean_mv") and video.MS_SSIM_COLUMNS == ("ms_ssim_y",)
    assert video.MS_SSIM_MIN_SIDE == msssim.MIN_SIDE and video.ms_ssim_part({"ms_ssim_y": 0.25}) == ", MS-SSIM-Y 0.250000"
    from fdn_hip import video_metrics
    assert video_metrics.RECORD_KEYS == ("psnr_y", "psnr_u", "psnr_v", "psnr_avg", "ssim_y", "mean_y", "mean_y_ref", "cut", "dmean", "dmean_ref")
    # a stream below 161 is refused with one line before anything touches the GPU (this machine may have none)
    small = b"YUV4MPEG2 W208 H160 F25:1 Ip A1:1 C420\n" + b"FRAME\n" + bytes(208 * 160 * 3 // 2)
    (tmp_path / "s.y4m").write_bytes(small)
    with pytest.raises(SystemExit) as e:
        video.main(["--ref", str(tmp_path / "s.y4m"), str(tmp_path / "s.y4m"), "--ms-ssim"])
    assert str(e.value.code) == "calculate_video_metrics.py: --ms-ssim: five scales need frames of at least 161x161, the streams are 208x160"

    # validate_fdn.py: absent unless given, the default namespace is what it was
    vbase = ["--fdn", "unused.pth", "--lq", str(rs / "[ab].png"), "--gt", str(gt / "*.png")]
    old = {"fdn", "lpnet", "lq", "gt", "variant", "ratio", "crop_border", "output", "csv", "batch", "device", "tile", "tile_overlap", "tile_ratio",
           "tile_blend", "ensemble", "fourier", "fourier_bands", "pairs", "dest"}
    assert set(vars(validate.parse_args(vbase))) == old
    assert validate.parse_args(vbase + ["--ms-ssim"]).ms_ssim is True and set(vars(validate.parse_args(vbase + ["--ms-ssim"]))) == old | {"ms_ssim"}
    with pytest.raises(SystemExit):
        validate.parse_args(vbase + ["--ms-ssim", "yes"])
    assert validate.csv_header(validate.parse_args(vbase)) == "frame,psnr,ssim,ratio"
    assert validate.csv_header(validate.parse_args(vbase + ["--ms-ssim"])) == "frame,psnr,ssim,ratio,ms_ssim"
    assert validate.csv_header(validate.parse_args(vbase + ["--ms-ssim", "--sharpness", "--lowlight", "--correct", "gt_mean"])) == \
        "frame,psnr,ssim,ratio,loe,deltae,psnr_corr,ssim_corr,edge,gmsd,grad_ratio,ms_ssim"
