"""CPU: PIQE's definition and host side.  The ordered numpy restatement of tests/piqe_ref.py (what the device must reproduce bit for
bit) is held to the plain one (scipy's correlate1d, np.var and np.std(ddof=1) on slices), block by block; its properties are checked
exactly; the entry points of include/fdn_piqe.h in libfdn_piqe.so are checked for their version, their generated prototype table,
fdn_piqe_dims and every argument refusal before any launch; and the three command lines for their arguments.  No GPU compute.

How the two forms are compared, and why.  They sum in different orders, so they differ by rounding.  A block's variance and its csd
must agree within 1e-10 relative, |a - b| <= 1e-10 * |b|, whatever their size.  The smallest segment std is held to the same bound
wherever it can be: the MSCN values it is formed from carry an ABSOLUTE error of about 1e-12 (codes up to 255, so m2 - mu * mu cancels
about 16 bits), whatever their size, and the std of six of them inherits it - the std of a flat segment is pure rounding noise (1e-15 in
one form, 0 or 1e-17 in the other) and has no relative error to speak of, and one of 0.004 already misses 1e-10 relative by a hair.  So
for this one quantity "relative" is taken against the larger of the value and the threshold it is compared with, 0.1:
|a - b| <= 1e-10 * max(|b|, 0.1), which is the plain relative bound for every std at or above the threshold.  Classes must be equal for
every block none of whose deciding quantities lies within 1e-9 relative of its threshold (v against 0.1, the smallest std against 0.1,
sigma against 2 beta); up to 1 % of the blocks might be left out that way, but the fixtures were chosen so that the ordered form leaves
out NO block, which the test asserts.  The plain form classifies with its own lines (piqe_ref.classify_plain), so that a wrong decision
formula in the ordered form shows here too."""
import ctypes
import importlib.util
import math
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as entry  # noqa: F401  (puts the package on sys.path)
import piqe_ref as ref
from fdn_hip import piqe  # noqa: E402  (the module under test: without it nothing here has a subject)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fdn-tip2025_amd")
NAMES = ["fdn_piqe_abi_version", "fdn_piqe_dims", "fdn_piqe_ws", "fdn_piqe_u8", "fdn_piqe_luma"]
# one block; padding on both sides; odd; every class; one pixel and one block past the 32 x 64 tile
SHAPES = [(16, 16), (17, 33), (47, 95), (161, 257), (33, 65), (48, 80)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(piqe.lib_path()):
        entry.build()
    return piqe.lib()


# ---- (a) the table and the header -----------------------------------------------------------------------------------------------------
def test_version_and_generated_table(lib, monkeypatch):
    spec = importlib.util.spec_from_file_location("gen_abi_table", os.path.join(ROOT, "tools", "gen_abi_table.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    from fdn_hip import _abi_piqe as table
    protos, names, members, versions = gen.build_table(headers=["fdn_piqe.h"])
    assert table.PROTOTYPES == protos and table.ARG_NAMES == names and list(protos) == members["fdn_piqe.h"] == NAMES
    assert table.VERSION == versions["fdn_piqe.h"] == ("fdn_piqe_abi_version", 1)
    assert "fdn_piqe.h" not in gen.HEADERS                                         # the one table of libfdn_hip.so stays what it was
    assert lib.fdn_piqe_abi_version() == 1 == piqe.ABI_VERSION
    assert lib.fdn_piqe_ws.restype == ctypes.c_long
    assert lib.fdn_piqe_u8.argtypes == [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 7
    assert lib.fdn_piqe_luma.argtypes == [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_long] + [ctypes.c_void_p] * 7
    assert table.ARG_NAMES["fdn_piqe_u8"] == ["img", "B", "h", "w", "bgr", "taps7", "mscn", "var", "cls", "ws", "out", "stream"]
    assert table.ARG_NAMES["fdn_piqe_luma"] == ["frames", "B", "h", "w", "bits", "stride", "taps7", "mscn", "var", "cls", "ws", "out", "stream"]
    header = open(os.path.join(ROOT, "include", "fdn_piqe.h")).read()
    assert f"FDN_PIQE_BLOCK = {piqe.BLOCK}, FDN_PIQE_TILE_H = {piqe.TILE_H}, FDN_PIQE_TILE_W = {piqe.TILE_W}" in header
    assert f"FDN_PIQE_ACTIVE = {piqe.ACTIVE}, FDN_PIQE_WNDC = {piqe.WNDC}, FDN_PIQE_WNC = {piqe.WNC}" in header
    assert (piqe.BLOCK, piqe.TILE_H, piqe.TILE_W, piqe.ACTIVE, piqe.WNDC, piqe.WNC) == (ref.BLOCK, ref.TILE_H, ref.TILE_W, ref.ACTIVE, ref.WNDC, ref.WNC)
    for sentence in ("THIS TEXT IS THE DEFINITION", "this header wins", "No comparison against MATLAB\n * or pyiqa has been made", "exactly 100.0"):
        assert sentence in header, sentence
    assert np.array_equal(piqe._TAPS, ref.taps()) and piqe._TAPS.dtype == np.float64 and piqe._TAPS.shape == (7,)
    assert abs(piqe._TAPS.sum() - 1.0) < 1e-15 and np.array_equal(piqe._TAPS, piqe._TAPS[::-1])
    # none of the other libraries holds these entry points
    import fdn_hip
    from fdn_hip import msssim, sharpness
    for other in (fdn_hip.lib(), msssim.lib(), sharpness.lib()):
        assert not hasattr(other, "fdn_piqe_u8")
    # a library of another version is refused with the sentence of fdn_hip.lib()
    monkeypatch.setattr(piqe, "_lib", None)
    monkeypatch.setattr(piqe, "ABI_VERSION", 2)
    with pytest.raises(ImportError, match=r"libfdn_piqe\.so has piqe ABI version 1, this binding needs 2: rebuild with build\.sh"):
        piqe.lib()
    assert piqe._lib is None


def test_dims_rule(lib):
    for h, w in SHAPES + [(1, 1), (720, 1280), (1080, 1920), (15, 2 ** 31 // 16 - 16), (46336, 46336)]:
        d = piqe.piqe_dims(h, w)
        assert (d["H"], d["W"]) + d["blocks"] + d["tiles"] == ref.dims(h, w), (h, w)
    assert piqe.piqe_dims(17, 33) == {"H": 32, "W": 48, "blocks": (2, 3), "tiles": (1, 1)}
    assert piqe.piqe_dims(720, 1280) == {"H": 720, "W": 1280, "blocks": (45, 80), "tiles": (23, 20)}
    arr = (ctypes.c_int * 6)(*[-7] * 6)
    for h, w in [(0, 16), (16, 0), (-1, 500), (46341, 46341), (16, 2 ** 31 // 16), (2 ** 31 - 1, 1)]:
        assert lib.fdn_piqe_dims(h, w, arr) == 1 and list(arr) == [-7] * 6, (h, w)
    assert lib.fdn_piqe_dims(200, 200, None) == 1
    from fdn_hip import FdnHipError
    with pytest.raises(FdnHipError, match="refuses 0x400"):
        piqe.piqe_dims(0, 400)


GOOD = dict(B=2, h=50, w=70)
BAD = [dict(B=0), dict(B=-1), dict(h=0), dict(w=-3), dict(h=46341, w=46341), dict(h=2 ** 31 - 1, w=16)]


def check_argument_errors(lib):
    """every refusal of include/fdn_piqe.h returns its code before any launch: FDN_ERR_ARG = 1, FDN_ERR_UNSUPPORTED = 4 (the pointers are
    never dereferenced - taps7 is read only after the checks - and a machine without a GPU has nothing to launch on); the workspace
    query answers 0 to the same sizes"""
    p = ctypes.c_void_p(64)                                                        # never dereferenced

    def u8(ptrs=None, bgr=0, **kw):
        a = {**GOOD, **kw}
        q = dict(img=p, taps=p, mscn=None, var=None, cls=None, ws=p, out=p)
        q.update(ptrs or {})
        return lib.fdn_piqe_u8(q["img"], a["B"], a["h"], a["w"], bgr, q["taps"], q["mscn"], q["var"], q["cls"], q["ws"], q["out"], None)

    def luma(ptrs=None, bits=8, stride=None, **kw):
        a = {**GOOD, **kw}
        q = dict(img=p, taps=p, mscn=None, var=None, cls=None, ws=p, out=p)
        q.update(ptrs or {})
        stride = a["h"] * a["w"] * 3 // 2 if stride is None else stride
        return lib.fdn_piqe_luma(q["img"], a["B"], a["h"], a["w"], bits, stride, q["taps"], q["mscn"], q["var"], q["cls"], q["ws"], q["out"], None)

    for bad in BAD:
        assert u8(**bad) == 1 and u8(bgr=1, **bad) == 1 and luma(**bad) == 1 and luma(bits=10, **bad) == 1, bad
        a = {**GOOD, **bad}
        assert lib.fdn_piqe_ws(a["B"], a["h"], a["w"]) == 0, bad
    for k in ("img", "taps", "ws", "out"):
        assert u8({k: None}) == 1 and luma({k: None}) == 1, k
    for off in (1, 2, 4, 68):                                                       # ws not 8-byte aligned
        assert u8({"ws": ctypes.c_void_p(64 + off)}) == 1 and luma({"ws": ctypes.c_void_p(64 + off)}) == 1, off
    for bits in (0, 9, 12, 16):
        assert luma(bits=bits) == 1
    assert luma(stride=50 * 70 - 1) == 1                                            # frames that overlap their Y planes
    # more workgroups than a grid holds (2^24 - 1 of 256 threads): 33 x 65 has 2 x 2 tiles, and 2^22 images is the first count refused
    assert u8(B=2 ** 22, h=33, w=65) == 4 and luma(B=2 ** 22, h=33, w=65) == 4 and u8(B=2 ** 24, h=16, w=16) == 4
    assert u8(B=2 ** 29, h=33, w=65) == 4 and luma(B=2 ** 29, h=33, w=65) == 4 and luma(B=2 ** 29, h=33, w=65, bits=10) == 4
    # the workspace: two doubles per tile of every plane
    for B, h, w in [(1, 16, 16), (2, 50, 70), (3, 161, 257), (1, 720, 1280), (8, 33, 65)]:
        *_, ty, tx = ref.dims(h, w)
        assert lib.fdn_piqe_ws(B, h, w) == 2 * B * ty * tx, (B, h, w)
    assert lib.fdn_piqe_ws(1, 720, 1280) == 2 * 23 * 20


def test_entry_points_validate_arguments_without_gpu(lib):
    check_argument_errors(lib)


def test_module_refuses_without_a_device():
    from fdn_hip import FdnHipError
    z = np.zeros((20, 20, 3), np.uint8)
    for f in (piqe.piqe_u8, piqe.piqe_sums_u8):
        with pytest.raises(FdnHipError, match="takes uint8 images"):
            f(z.astype(np.float32))
        with pytest.raises(FdnHipError, match="takes uint8 images"):
            f(z[..., :2])
    from fdn_hip.harness import VideoFormat
    with pytest.raises(ValueError, match="at least 1x1, got 208x0"):
        piqe.PiqeScore(0, 208, VideoFormat("yuv420p"))
    assert math.isnan(piqe.PiqeScore(48, 80, VideoFormat("yuv420p")).summary()["piqe_y"])
    assert piqe.piqe_from_sums(0.0, 0) == 100.0 and piqe.piqe_from_sums(3.0, 7) == 50.0 == ref.score(3.0, 7)
    assert piqe.piqe_line({"piqe": 12.5, "d": 1.0, "nhsa": 7}) == "PIQE: 12.500000 (7 active blocks)"
    src = open(os.path.join(PKG, "fdn_hip", "piqe.py")).read()
    assert "oracle" not in src and "tests" not in src.replace("tests/", "")           # the product path stands without the yardsticks


# ---- (b) the ordered form against the plain one -----------------------------------------------------------------------------------------
def fixtures():
    out = [("quadrants %dx%d" % s, ref.plane_u8(ref.quadrants(*s))) for s in SHAPES]
    out += [("texture " + k, ref.plane_u8(v)) for k, v in ref.degradations(160, 256).items()]
    out += [("luma %d bit %dx%d" % (b, h, w), ref.plane_luma(ref.luma_frames(1, h, w, b)[0], h, w, b)) for b in (8, 10) for h, w in ((48, 80), (162, 258))]
    return out


def undecided(r):
    """blocks one of whose deciding quantities lies within 1e-9 relative of its threshold"""
    with np.errstate(all="ignore"):
        near = (np.abs(r["v"] - ref.T_ACTIVE) <= 1e-9 * ref.T_ACTIVE) | (np.abs(r["minseg"] - ref.T_SEG) <= 1e-9 * ref.T_SEG)
        return near | (np.abs(r["sigma"] - 2.0 * r["beta"]) <= 1e-9 * r["sigma"])


def test_ordered_form_against_the_plain_one():
    seen = np.zeros(8, dtype=np.int64)
    for name, (code, q) in fixtures():
        o, p = ref.plane_result(code, q), ref.plane_result_plain(code, q)
        assert o["mscn"].shape == p["mscn"].shape == ref.dims(*code.shape)[:2]
        assert float(np.abs(o["mscn"] - p["mscn"]).max()) < 1e-10, name
        for k in ("v", "minseg", "csd"):
            ok = np.isfinite(p[k])
            assert np.array_equal(ok, np.isfinite(o[k])), (name, k)
            diff, size = np.abs(o[k][ok] - p[k][ok]), np.abs(p[k][ok])
            bound = 1e-10 * (np.maximum(size, ref.T_SEG) if k == "minseg" else size)    # the one floor: see the head of this file
            print(f"{name}: {k} worst {float((diff / np.maximum(bound, 1e-300)).max()):.3g} of the bound")
            assert (diff <= bound).all(), (name, k, float((diff / np.maximum(bound, 1e-300)).max()))
        out = undecided(o)
        assert out.sum() == 0, (name, int(out.sum()))                                 # the fixtures leave no block out
        assert np.array_equal(o["cls"], p["cls"]), name
        assert o["nhsa"] == p["nhsa"] and abs(o["D"] - p["D"]) <= 1e-10 * max(1.0, abs(p["D"])) and abs(o["piqe"] - p["piqe"]) < 1e-9, name
        seen += np.bincount(o["cls"].ravel(), minlength=8)
    assert all(seen[c] > 20 for c in (0, 1, 3, 5, 7)) and seen[[2, 4, 6]].sum() == 0     # every class is met; none without the active bit


def test_every_class_is_present_at_161x257():
    cls = ref.result_u8(ref.quadrants(161, 257))["cls"]
    assert cls.shape == (11, 17)
    for c in (0, 1, 3, 5, 7):
        assert (cls == c).sum() >= 0.03 * cls.size, (c, int((cls == c).sum()))


# ---- (c) properties, exact ----------------------------------------------------------------------------------------------------------------
def test_flat_image_scores_exactly_100():
    for value in (0, 37, 255):
        r = ref.plane_result(*ref.plane_u8(np.full((40, 50, 3), value, np.uint8)))
        assert r["nhsa"] == 0 and r["D"] == 0.0 and r["piqe"] == 100.0 and not r["cls"].any()


def test_padding_is_replication():
    """a 17 x 33 image equals its own replicate-padded 32 x 48 version, bit for bit"""
    a = ref.quadrants(17, 33)
    b = np.pad(a, ((0, 15), (0, 15), (0, 0)), mode="edge")
    ra, rb = ref.result_u8(a), ref.result_u8(b)
    assert b.shape == (32, 48, 3) and np.array_equal(ra["mscn"], rb["mscn"]) and np.array_equal(ra["v"], rb["v"])
    assert np.array_equal(ra["cls"], rb["cls"]) and (ra["D"], ra["nhsa"], ra["piqe"]) == (rb["D"], rb["nhsa"], rb["piqe"])


def test_bgr_flag_and_ten_bit_quarters():
    a = ref.quadrants(47, 95)
    flip = np.ascontiguousarray(a[..., ::-1])
    assert np.array_equal(ref.plane_u8(a)[0], ref.plane_u8(flip, bgr=True)[0]) and not np.array_equal(ref.plane_u8(a)[0], ref.plane_u8(flip)[0])
    assert ref.result_u8(a)["piqe"] == ref.result_u8(flip, bgr=True)["piqe"]
    g = np.arange(256, dtype=np.uint8)
    assert np.array_equal(ref.plane_u8(np.stack([g, g, g], -1)[None])[0][0], g)         # a gray image's code is its plane
    assert ref.plane_u8(np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [1, 1, 0]]], np.uint8))[0].tolist() == [[76, 150, 29, 1]]
    c = ref.plane_u8(a)[0]
    r8 = ref.plane_result(c, 1)
    r10 = ref.plane_result(*ref.plane_luma((4 * c).astype(np.uint16).ravel(), 47, 95, 10))
    assert np.array_equal(r8["mscn"], r10["mscn"]) and (r8["D"], r8["nhsa"], r8["piqe"]) == (r10["D"], r10["nhsa"], r10["piqe"])
    y = np.array([0, 1023, 1024, 65535] * 4, dtype=np.uint16)
    assert ref.plane_luma(np.concatenate([y, y[:8]]), 4, 4, 10)[0].ravel().tolist() == [0, 1023, 1023, 1023] * 4


def test_degradations_are_ranked():
    """on the smooth texture: clean < noise of sigma 10 < noise of sigma 25 < its 8 x 8 block means (17.1 < 43.1 < 65.8 < 85.9)"""
    s = {k: ref.result_u8(v)["piqe"] for k, v in ref.degradations(160, 256).items()}
    print(s)
    assert 0.0 < s["clean"] < s["noise10"] < s["noise25"] < s["blocks"] < 100.0
    assert s["clean"] < 25.0 and s["blocks"] > 75.0


def test_fold_order():
    """the header's order of D: tile partials row-major within the tile, slots walking tiles t, t + 256, ..., then the tree"""
    g = np.random.default_rng(3)
    d, act = g.standard_normal((45, 80)), g.random((45, 80)) < 0.7                    # 23 x 20 = 460 tiles: slots 0 .. 203 take two
    D, n = ref.fold_ordered(d, act)
    assert n == int(act.sum()) and abs(D - d[act].sum()) < 1e-10
    def chain(terms):                                                                # one addition at a time (the built-in sum compensates)
        s = 0.0
        for t in terms:
            s = s + float(t)
        return s

    parts = [chain(d[i, j] for i in range(2 * ty, min(2 * ty + 2, 45)) for j in range(4 * tx, 4 * tx + 4) if act[i, j])
             for ty in range(23) for tx in range(20)]
    slot = [chain(parts[t::256]) for t in range(256)]
    while len(slot) > 1:
        half = len(slot) // 2
        slot = [slot[t] + slot[t + half] for t in range(half)]
    assert D == slot[0]


# ---- (d) the command lines ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clis():
    sys.path.insert(0, PKG)
    import calculate_piqe
    import calculate_video_metrics
    import validate_fdn
    return calculate_piqe, calculate_video_metrics, validate_fdn


def test_command_lines_parse_their_arguments(clis, tmp_path, capsys):
    from PIL import Image
    score, video, validate = clis
    g = np.random.default_rng(0)
    gt, rs = tmp_path / "gt", tmp_path / "rs"
    gt.mkdir(); rs.mkdir()
    for n in "ab":
        Image.fromarray(g.integers(0, 256, (16, 20, 3), dtype=np.uint8)).save(gt / f"{n}.png")
        Image.fromarray(g.integers(0, 256, (16, 20, 3), dtype=np.uint8)).save(rs / f"{n}.png")
    Image.fromarray(g.integers(0, 256, (16, 20), dtype=np.uint8)).save(rs / "c.png")
    Image.fromarray(g.integers(0, 256, (16, 20, 4), dtype=np.uint8)).save(rs / "d.png")
    a = score.parse_args(["--input", str(rs)])
    assert [os.path.basename(p) for p in a.paths] == ["a.png", "b.png", "c.png", "d.png"]
    assert (a.batch, a.device, a.drop_alpha, a.csv, a.masks) == (8, "cuda:0", False, None, None)
    a = score.parse_args(["--input", str(rs / "[ab].png"), "--batch", "3", "--csv", "x.csv", "--masks", "m", "--drop_alpha", "--device", "cuda:1"])
    assert [os.path.basename(p) for p in a.paths] == ["a.png", "b.png"] and (a.batch, a.device, a.drop_alpha, a.csv, a.masks) == (3, "cuda:1", True, "x.csv", "m")
    for argv in ([], ["--input", str(rs / "*.jpg")], ["--input", str(rs), "--batch", "0"]):
        with pytest.raises(SystemExit):
            score.parse_args(argv)
    # the loader: R, G, B as PIL gives them; greyscale in all three channels; alpha refused unless dropped
    assert score.load_rgb(str(rs / "a.png")).shape == (16, 20, 3) and np.array_equal(score.load_rgb(str(rs / "a.png")), np.array(Image.open(rs / "a.png")))
    c = score.load_rgb(str(rs / "c.png"))
    assert c.shape == (16, 20, 3) and np.array_equal(ref.plane_u8(c)[0], np.array(Image.open(rs / "c.png")))
    with pytest.raises(ValueError, match="alpha channel"):
        score.load_rgb(str(rs / "d.png"))
    assert np.array_equal(score.load_rgb(str(rs / "d.png"), drop_alpha=True), np.array(Image.open(rs / "d.png"))[..., :3])
    # the masks: every block its 16 x 16 pixels, cut to the image
    m = score.mask_images(np.array([[1, 3], [5, 0]], np.uint8), 20, 30)
    assert sorted(m) == ["active", "wnc", "wndc"] and all(v.shape == (20, 30) and v.dtype == np.uint8 for v in m.values())
    assert m["active"][0, 0] == 255 and m["active"][19, 29] == 0 and m["active"][16, 0] == 255 and m["active"][15, 16] == 255
    assert m["wndc"][0, 16] == 255 and m["wndc"][0, 15] == 0 and m["wnc"][16, 15] == 255 and m["wnc"][15, 15] == 0

    # calculate_video_metrics.py: --piqe works with and without --ref
    assert video.parse_args(["out.y4m", "--piqe"]).piqe is True and video.parse_args(["--ref", "gt.y4m", "out.y4m", "--piqe"]).piqe is True
    assert video.parse_args(["--ref", "gt.y4m", "out.y4m"]).piqe is False
    assert video.PIQE_COLUMNS == ("piqe_y", "piqe_y_ref")
    assert video.piqe_part({"piqe_y": 12.5}) == ", PIQE-Y 12.500000" and video.piqe_part({"piqe_y": 12.5}, {"piqe_y": 3.0}) == ", PIQE-Y 12.500000 (ref 3.000000)"

    # validate_fdn.py: absent unless given, the default namespace is what it was
    vbase = ["--fdn", "unused.pth", "--lq", str(rs / "[ab].png"), "--gt", str(gt / "*.png")]
    old = {"fdn", "lpnet", "lq", "gt", "variant", "ratio", "crop_border", "output", "csv", "batch", "device", "tile", "tile_overlap", "tile_ratio",
           "tile_blend", "ensemble", "fourier", "fourier_bands", "pairs", "dest"}
    assert set(vars(validate.parse_args(vbase))) == old
    assert validate.parse_args(vbase + ["--piqe"]).piqe is True and set(vars(validate.parse_args(vbase + ["--piqe"]))) == old | {"piqe"}
    with pytest.raises(SystemExit):
        validate.parse_args(vbase + ["--piqe", "yes"])
    assert validate.csv_header(validate.parse_args(vbase)) == "frame,psnr,ssim,ratio"
    assert validate.csv_header(validate.parse_args(vbase + ["--piqe"])) == "frame,psnr,ssim,ratio,piqe,piqe_gt"
    assert validate.csv_header(validate.parse_args(vbase + ["--piqe", "--ms-ssim", "--sharpness"])) == "frame,psnr,ssim,ratio,edge,gmsd,grad_ratio,ms_ssim,piqe,piqe_gt"
