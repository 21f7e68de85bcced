"""CPU: exposure fusion's definitions and host side.  The float64 restatement of tests/fusion_ref.py is held to the properties that make it
a fusion (one rendering, or K equal ones, fuse to the rendering; the weight planes sum to 1 at every level; up(down(.)) keeps a constant;
a permutation of the renderings permutes the weights); the entry points of include/fdn_fusion.h in libfdn_fusion.so are checked for their
version, their generated prototype table, fdn_fusion_dims, fdn_fusion_ws and every argument refusal before any launch; the bracket
helpers; and the command lines for their argument errors.  No GPU compute."""
import ctypes
import importlib.util
import itertools
import math
import os
import sys

import numpy as np
import pytest
import torch

import __graft_entry__ as entry  # noqa: F401  (puts the package on sys.path)
import fusion_ref as ref
from fdn_hip import fusion  # noqa: E402  (the module under test: without it nothing here has a subject)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fdn-tip2025_amd")
NAMES = ["fdn_fusion_abi_version", "fdn_fusion_dims", "fdn_fusion_ws", "fdn_fuse_weights", "fdn_fuse_pyramid", "fdn_pyr_down", "fdn_pyr_up"]
SHAPES = [(1, 1), (1, 7), (6, 1), (2, 2), (2, 3), (3, 5), (4, 4), (5, 8), (9, 9), (13, 22), (33, 31)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(fusion.lib_path()):
        entry.build()
    return fusion.lib()


# ---------------------------------------------------------------------------------------------------------------------------------
# the float64 restatement, without the clamp, within 1e-12
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_one_rendering_fuses_to_itself(shape):
    img = ref.scene(*shape, K=1, seed=1).astype(np.float64) * 3 - 1                     # values outside [0, 1] too: nothing is clamped
    got = ref.fuse_pyramid(img, ref.weights(img, clamp=False), dtype=np.float64, clamp=False)
    assert np.abs(got - img[0]).max() <= 1e-12


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("K", [2, 5, 16])
def test_equal_renderings_fuse_to_the_rendering(shape, K):
    one = ref.scene(*shape, K=1, seed=2).astype(np.float64)
    imgs = np.repeat(one, K, axis=0)
    wts = ref.weights(imgs, clamp=False)
    assert np.abs(wts - 1.0 / K).max() <= 1e-12
    assert np.abs(ref.fuse_pyramid(imgs, wts, dtype=np.float64, clamp=False) - one[0]).max() <= 1e-12


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("exponents", [(1, 1, 1), (0, 0, 1), (0.5, 2, 1), (0, 0, 0)])
def test_weight_planes_sum_to_one_at_every_level(shape, exponents):
    imgs = ref.scene(*shape, K=4, seed=3).astype(np.float64)
    wts = ref.weights(imgs, exponents, clamp=False)
    pyr = ref.weight_pyramid(wts)
    assert len(pyr) == ref.levels(*shape) + 1 and [p.shape[1:] for p in pyr] == ref.sizes(*shape)
    for level in pyr:
        assert (level >= 0).all() and np.abs(level.sum(axis=0) - 1.0).max() <= 1e-12
    if exponents == (0, 0, 0):
        assert np.abs(wts - 0.25).max() <= 1e-12                                       # every factor left out: 1 + 1e-12 each


@pytest.mark.parametrize("h", range(1, 10))
@pytest.mark.parametrize("w", range(1, 10))
def test_up_of_down_keeps_a_constant(h, w):
    x = np.full((2, h, w), 0.3713, dtype=np.float64)
    d = ref.down(x)
    assert d.shape == (2, (h + 1) // 2, (w + 1) // 2) and np.abs(d - 0.3713).max() <= 1e-12
    assert np.abs(ref.up(d, h, w) - 0.3713).max() <= 1e-12
    x32 = np.full((1, h, w), 0.3713, dtype=np.float32)                                 # an axis of length 1 returns its sample untouched
    if h == 1 and w == 1:
        assert np.array_equal(ref.down(x32), x32) and np.array_equal(ref.up(x32, 1, 1), x32)


def test_a_permutation_of_the_renderings_permutes_the_weights():
    imgs = ref.scene(13, 22, K=4, seed=4).astype(np.float64)
    base = ref.weights(imgs, clamp=False)
    for perm in itertools.islice(itertools.permutations(range(4)), 1, None, 5):
        got = ref.weights(imgs[list(perm)], clamp=False)
        assert np.abs(got - base[list(perm)]).max() <= 1e-12


def test_reflect_and_sizes():
    assert ref.reflect([-3, -2, -1, 0, 1, 2, 3, 4, 5, 6, 7], 4).tolist() == [3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1]
    assert ref.reflect([-2, -1, 0, 1, 2, 3], 2).tolist() == [0, 1, 0, 1, 0, 1] and ref.reflect([-2, 0, 5], 1).tolist() == [0, 0, 0]
    assert ref.sizes(5, 9) == [(5, 9), (3, 5), (2, 3)] and ref.levels(1, 100) == 0 and ref.levels(720, 1280) == 9
    lo = ref.weights(ref.scene(6, 7, K=3, seed=5))                                     # the clamp acts before anything else
    assert np.array_equal(lo, ref.weights(ref.clamp01(ref.scene(6, 7, K=3, seed=5)), clamp=False))


# ---------------------------------------------------------------------------------------------------------------------------------
# the library's host side
# ---------------------------------------------------------------------------------------------------------------------------------
def test_version_and_generated_table(lib, monkeypatch):
    spec = importlib.util.spec_from_file_location("gen_abi_table", os.path.join(ROOT, "tools", "gen_abi_table.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    from fdn_hip import _abi_fusion as table
    protos, names, members, versions = gen.build_table(headers=["fdn_fusion.h"])
    assert table.PROTOTYPES == protos and table.ARG_NAMES == names and list(protos) == members["fdn_fusion.h"] == NAMES
    assert table.VERSION == versions["fdn_fusion.h"] == ("fdn_fusion_abi_version", 1)
    assert "fdn_fusion.h" not in gen.HEADERS                                       # the one table of libfdn_hip.so stays what it was
    assert lib.fdn_fusion_abi_version() == 1 == fusion.ABI_VERSION
    assert lib.fdn_fusion_ws.restype == ctypes.c_long
    assert lib.fdn_fuse_weights.argtypes == [ctypes.c_void_p] * 2 + [ctypes.c_int] * 5 + [ctypes.c_double] * 3 + [ctypes.c_void_p]
    assert lib.fdn_fuse_pyramid.argtypes == [ctypes.c_void_p] * 4 + [ctypes.c_int] * 5 + [ctypes.c_void_p]
    assert table.ARG_NAMES["fdn_fuse_weights"] == ["imgs", "weights", "K", "h", "w", "H", "W", "wc", "ws", "we", "stream"]
    header = open(os.path.join(ROOT, "include", "fdn_fusion.h")).read()
    assert f"FDN_FUSION_MAX_K = {fusion.MAX_K}, FDN_FUSION_MAX_LEVELS = {fusion.MAX_LEVELS}, FDN_FUSION_TILE = {fusion.TILE}" in header
    assert (fusion.MAX_K, fusion.MAX_LEVELS, fusion.TILE) == (ref.MAX_K, ref.MAX_LEVELS, ref.TILE)
    assert repr(2 * 0.2 ** 2) == "0.08000000000000002" == repr(ref.SIGMA2) and "/ 0.08000000000000002)" in header
    # none of the other libraries holds these entry points
    import fdn_hip
    from fdn_hip import correct, sharpness
    for other in (fdn_hip.lib(), correct.lib(), sharpness.lib()):
        assert not hasattr(other, "fdn_fuse_pyramid") and not hasattr(other, "fdn_pyr_down")
    # a library of another version is refused with the sentence of fdn_hip.lib()
    monkeypatch.setattr(fusion, "_lib", None)
    monkeypatch.setattr(fusion, "ABI_VERSION", 2)
    with pytest.raises(ImportError, match=r"libfdn_fusion\.so has fusion ABI version 1, this binding needs 2: rebuild with build\.sh"):
        fusion.lib()
    assert fusion._lib is None


def test_dims_rule(lib):
    for h in range(1, 71):
        for w in range(1, 71):
            L, sizes = fusion.dims(h, w)
            assert L == ref.levels(h, w) == int(math.floor(math.log2(min(h, w)))) and sizes == ref.sizes(h, w)
            assert len(sizes) == L + 1 and all(b == ((a[0] + 1) // 2, (a[1] + 1) // 2) for a, b in zip(sizes, sizes[1:]))
    assert fusion.dims(720, 1280)[0] == 9 and fusion.dims(46340, 46340)[0] == 15 and fusion.dims(1, 2 ** 31 - 1)[0] == 0
    L = ctypes.c_int(-7)
    for h, w in [(0, 4), (4, 0), (-1, 4), (4, -2), (46341, 46341), (2, 2 ** 30)]:
        assert lib.fdn_fusion_dims(h, w, ctypes.byref(L)) == 1 and L.value == -7
    assert lib.fdn_fusion_dims(4, 4, None) == 1
    from fdn_hip import FdnHipError
    with pytest.raises(FdnHipError, match="fdn_fusion_dims"):
        fusion.dims(0, 3)


GOOD = dict(K=3, h=40, w=50, H=64, W=64)
BAD = [dict(K=0), dict(K=-1), dict(K=17), dict(h=0), dict(h=-4), dict(w=0), dict(w=-1), dict(H=39), dict(W=49),
       dict(h=46341, w=46341, H=46341, W=46341), dict(h=2 ** 31 - 1, w=2, H=2 ** 31 - 1, W=2)]


def check_argument_errors(lib):
    """every refusal of include/fdn_fusion.h returns its code before any launch: FDN_ERR_ARG = 1, FDN_ERR_UNSUPPORTED = 4 (the pointers
    are never dereferenced, and a machine without a GPU has nothing to launch on); fdn_fusion_ws answers -1 to the same sizes"""
    p = ctypes.c_void_p(64)                                                        # never dereferenced

    def wts(ptrs=None, e=(1.0, 1.0, 1.0), **kw):
        a = {**GOOD, **kw}
        q = dict(imgs=p, weights=p)
        q.update(ptrs or {})
        return lib.fdn_fuse_weights(q["imgs"], q["weights"], a["K"], a["h"], a["w"], a["H"], a["W"], e[0], e[1], e[2], None)

    def pyr(ptrs=None, **kw):
        a = {**GOOD, **kw}
        q = dict(imgs=p, weights=p, out=p, work=p)
        q.update(ptrs or {})
        return lib.fdn_fuse_pyramid(q["imgs"], q["weights"], q["out"], q["work"], a["K"], a["h"], a["w"], a["H"], a["W"], None)

    def down(ptrs=None, clamp=0, **kw):
        a = {**GOOD, **kw}
        q = {"in": p, "out": p}
        q.update(ptrs or {})
        return lib.fdn_pyr_down(q["in"], q["out"], a["K"], a["h"], a["w"], a["H"], a["W"], clamp, None)

    def up(ptrs=None, **kw):
        a = {**GOOD, **kw}
        q = {"in": p, "out": p}
        q.update(ptrs or {})
        return lib.fdn_pyr_up(q["in"], q["out"], a["K"], a["h"], a["w"], None)

    for bad in BAD:
        a = {**GOOD, **bad}
        assert wts(**bad) == 1 and pyr(**bad) == 1, bad
        if "K" in bad:
            assert lib.fdn_fusion_ws(a["K"], a["h"], a["w"]) == -1, bad
            if bad["K"] <= 0:                                                       # C planes: any positive count
                assert down(**bad) == 1 and up(**bad) == 1, bad
        elif "H" in bad and "h" not in bad or "W" in bad and "w" not in bad:
            assert down(**bad) == 1, bad                                             # the crop does not fit its rows
        else:
            assert down(**bad) == 1 and up(**bad) == 1 and lib.fdn_fusion_ws(a["K"], a["h"], a["w"]) == -1, bad
    for k in ("imgs", "weights"):
        assert wts({k: None}) == 1 and pyr({k: None}) == 1, k
    assert pyr({"out": None}) == 1 and pyr({"work": None}) == 1
    for off in (1, 2, 4, 8, 68):                                                    # work not 16-byte aligned
        assert pyr({"work": ctypes.c_void_p(64 + off)}) == 1, off
    for k in ("in", "out"):
        assert down({k: None}) == 1 and up({k: None}) == 1, k
    for e in ((-1.0, 1.0, 1.0), (1.0, -1e-300, 1.0), (1.0, 1.0, float("nan")), (float("inf"), 1.0, 1.0), (1.0, float("-inf"), 1.0)):
        assert wts(e=e) == 1, e
    # more workgroups than a grid holds, more planes than a grid's second axis
    assert down(K=2 ** 30, h=130, w=2, H=130, W=2) == 4 and up(K=65536) == 4
    # the workspace: (4 K + 3) floats per sample of levels 1 .. L; none for a frame with a 1-pixel axis
    assert lib.fdn_fusion_ws(3, 1, 50) == 0 and lib.fdn_fusion_ws(16, 77, 1) == 0
    assert lib.fdn_fusion_ws(2, 2, 2) == 4 * 11 * 1 and lib.fdn_fusion_ws(1, 5, 9) == 4 * 7 * (15 + 6)
    n = sum(a * b for a, b in ref.sizes(720, 1280)[1:])
    assert lib.fdn_fusion_ws(3, 720, 1280) == 4 * 15 * n and lib.fdn_fusion_ws(16, 720, 1280) == 4 * 67 * n


def test_entry_points_validate_arguments_without_gpu(lib):
    check_argument_errors(lib)


def test_module_refuses_without_a_device(lib):
    from fdn_hip import FdnHipError
    z = torch.zeros(3, 3, 8, 8)
    for f in (lambda: fusion.weights(z, 8, 8), lambda: fusion.fuse(z, 8, 8), lambda: fusion.fuse_pyramid(z, torch.zeros(3, 8, 8), 8, 8),
              lambda: fusion.pyr_down(z[0]), lambda: fusion.pyr_up(z[0], 16, 16)):
        with pytest.raises(FdnHipError, match="must live on a ROCm device"):
            f()
    with pytest.raises(FdnHipError, match=r"imgs must be fp32 \[K,3,H,W\]"):
        fusion.weights(torch.zeros(3, 8, 8), 8, 8)
    with pytest.raises(FdnHipError, match="17 renderings, 1 to 16"):
        fusion.fuse(torch.zeros(17, 3, 8, 8), 8, 8)
    with pytest.raises(FdnHipError, match="cannot read 9x8"):
        fusion.weights(z, 9, 8)
    with pytest.raises(FdnHipError, match="pyr_up to 5x5 needs planes of 3x3"):
        fusion.pyr_up(torch.zeros(1, 2, 3), 5, 5)
    with pytest.raises(ValueError, match="three finite numbers >= 0"):
        fusion.weights(z, 8, 8, exponents=(1, -1, 1))
    src = open(os.path.join(PKG, "fdn_hip", "fusion.py")).read()
    assert "oracle" not in src and "tests" not in src.replace("tests/", "")           # the product path stands without the yardsticks


def test_check_bracket_and_bracket_ratios():
    assert fusion.check_bracket([-1, 0, 1]) == (-1.0, 0.0, 1.0) and fusion.check_bracket((0.5,)) == (0.5,)
    assert fusion.check_bracket(range(16)) == tuple(float(v) for v in range(16))
    for bad in ((), range(17), (0, 0), (1, float("nan")), (float("inf"),), (1, "x"), 3, None, (-0.0, 0.0)):
        with pytest.raises(ValueError):
            fusion.check_bracket(bad)
    assert fusion.check_exponents((0, 0.5, 2)) == (0.0, 0.5, 2.0)
    for bad in ((1, 1), (1, 1, 1, 1), (1, -0.1, 1), (1, float("inf"), 1), (1, float("nan"), 1), "abc", None):
        with pytest.raises(ValueError):
            fusion.check_exponents(bad)
    ratio = torch.tensor([[0.3], [0.05]])
    got = fusion.bracket_ratios(ratio, (-1, 0, 1.5))
    assert got.shape == (2, 3, 1) and got.dtype == torch.float32
    want = ratio.reshape(2, 1, 1) * torch.tensor([2.0 ** 1, 2.0 ** 0, 2.0 ** -1.5], dtype=torch.float32).reshape(1, 3, 1)
    assert torch.equal(got, want)
    assert torch.equal(got[:, 1], ratio) and torch.equal(got[:, 0], ratio * 2)         # stop 0 is the ratio itself; a negative stop is darker
    assert (got[:, 2] < ratio).all()                                                    # a positive stop, a smaller ratio: brighter
    assert torch.equal(fusion.bracket_ratios(torch.tensor([[40.0]]), (-3,)), torch.tensor([[[320.0]]]))   # nothing is clamped
    assert "caller's business" in fusion.bracket_ratios.__doc__
    from fdn_hip import FdnHipError
    with pytest.raises(FdnHipError, match=r"needs ratio \[B,1\]"):
        fusion.bracket_ratios(torch.ones(2), (0,))


def test_harness_checks_the_bracket_before_anything_else():
    from fdn_hip import harness
    z = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    for kw in (dict(bracket=(0, 0)), dict(bracket=range(17)), dict(bracket=(0,), fusion=(1, 1)), dict(bracket=(0,), fusion=(1, -1, 1))):
        with pytest.raises(ValueError):
            harness.enhance_u8(None, None, z, ratio_mode="fixed", ratio=torch.ones(1, 1), **kw)
        with pytest.raises(ValueError):
            harness.validate_u8(None, None, z, z, **kw)
    with pytest.raises(ValueError, match="ratio_mode 'fixed' needs ratio"):
        harness.validate_u8(None, None, z, z, ratio_mode="fixed")


# ---------------------------------------------------------------------------------------------------------------------------------
# the command lines
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clis():
    sys.path.insert(0, PKG)
    import inference_fdn_lolblur
    import inference_fdn_multi_r
    import validate_fdn
    return inference_fdn_lolblur, inference_fdn_multi_r, validate_fdn


def test_command_lines_parse_their_arguments(clis, tmp_path, capsys):
    from PIL import Image
    driver, sweep, validate = clis
    base = ["--fdn", "f.pth", "--input", "x/*.png", "--output", "out"]
    a = driver.parse_driver_args("doc", argv=base + ["--lpnet", "l.pth"])[1]
    assert a.bracket is None and a.fusion_weights == (1.0, 1.0, 1.0) and a.ratio is None and a.lpnet == "l.pth"
    a = driver.parse_driver_args("doc", argv=base + ["--ratio", "0.25"])[1]                # --ratio makes --lpnet unnecessary
    assert a.ratio == 0.25 and a.lpnet is None
    a = driver.parse_driver_args("doc", argv=base + ["--ratio", "0.25", "--bracket", "-1,0,1", "--fusion-weights", "0,0.5,2"])[1]
    assert a.bracket == (-1.0, 0.0, 1.0) and a.fusion_weights == (0.0, 0.5, 2.0)
    assert driver.parse_driver_args("doc", argv=base + ["--lpnet", "l.pth", "--bracket=-2"])[1].bracket == (-2.0,)
    for argv in (base,                                                               # neither --lpnet nor --ratio
                 base + ["--ratio", "bright"], base + ["--ratio", "nan"], base + ["--ratio", "inf"],
                 base + ["--lpnet", "l.pth", "--bracket", "0,0"], base + ["--lpnet", "l.pth", "--bracket", ""],
                 base + ["--lpnet", "l.pth", "--bracket", ",".join(str(v) for v in range(17))],
                 base + ["--lpnet", "l.pth", "--bracket", "0,x"], base + ["--lpnet", "l.pth", "--bracket", "0,inf"],
                 base + ["--lpnet", "l.pth", "--fusion-weights", "1,1"], base + ["--lpnet", "l.pth", "--fusion-weights", "1,-1,1"]):
        with pytest.raises(SystemExit):
            driver.parse_driver_args("doc", argv=argv)
    capsys.readouterr()
    sbase = ["--fdn", "f.pth", "--input", "x.png"]
    a = sweep.parse_args(sbase)
    assert a.fuse is False and len(sweep.sweep_values(a.start, a.stop, a.step)) == 100
    a = sweep.parse_args(sbase + ["--fuse", "--start", "0.1", "--stop", "0.9", "--step", "0.05", "--fusion-weights", "1,0,1"])
    assert a.fuse is True and len(sweep.sweep_values(a.start, a.stop, a.step)) == 16 and a.fusion_weights == (1.0, 0.0, 1.0)
    with pytest.raises(SystemExit):
        sweep.parse_args(sbase + ["--fuse", "--start", "0.05", "--stop", "0.9", "--step", "0.05"])     # 17 values
    assert "--step" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        sweep.parse_args(sbase + ["--fuse"])                                         # the default grid has 100
    assert "--step" in capsys.readouterr().err
    g = np.random.default_rng(0)
    gt, lq = tmp_path / "gt", tmp_path / "lq"
    gt.mkdir(); lq.mkdir()
    for n in "ab":
        Image.fromarray(g.integers(0, 256, (16, 20, 3), dtype=np.uint8)).save(gt / f"{n}.png")
        Image.fromarray(g.integers(0, 256, (16, 20, 3), dtype=np.uint8)).save(lq / f"{n}.png")
    vbase = ["--fdn", "unused.pth", "--lq", str(lq / "*.png"), "--gt", str(gt / "*.png")]
    a = validate.parse_args(vbase)
    assert a.ratio == "gt" and not hasattr(a, "bracket") and not hasattr(a, "fusion_weights")   # absent unless given, as --lowlight
    assert validate.parse_args(vbase + ["--ratio", "lpnet", "--lpnet", "l.pth"]).ratio == "lpnet"
    a = validate.parse_args(vbase + ["--ratio", "0.3", "--bracket", "-1,0,1"])       # a number needs no --lpnet
    assert a.ratio == 0.3 and a.lpnet is None and a.bracket == (-1.0, 0.0, 1.0)
    assert validate.parse_args(vbase + ["--bracket", "0,1", "--fusion-weights", "2,2,0"]).fusion_weights == (2.0, 2.0, 0.0)
    assert validate.csv_header(a) == "frame,psnr,ssim,ratio"
    for argv in (vbase + ["--ratio", "lpnet"], vbase + ["--ratio", "fixed"], vbase + ["--ratio", "nan"], vbase + ["--bracket", "1,1"],
                 vbase + ["--fusion-weights", "1,1,1"]):                             # the exponents of nothing
        with pytest.raises(SystemExit):
            validate.parse_args(argv)
