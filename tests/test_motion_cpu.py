"""CPU: the definitions and the host side of the motion-compensated temporal consistency.  The numpy restatement of tests/motion_ref.py is
held to integers worked by hand (a 4 x 4 frame with R = 1, a flat frame), to the tie-break on stripes of period 4 and to a known shift of
random texture; the entry points of include/fdn_motion.h in libfdn_motion.so are checked for their version, their generated prototype
table and every argument refusal before any launch; MotionScore.add_host for its logic on synthetic integers; and the command line of
calculate_video_metrics.py for --motion.  No GPU compute."""
import ctypes
import importlib.util
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

import __graft_entry__ as entry  # noqa: F401  (puts the package on sys.path)
import motion_ref as ref
from fdn_hip import harness, motion  # noqa: E402  (the module under test: without it nothing here has a subject)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fdn-tip2025_amd")
NAMES = ["fdn_motion_abi_version", "fdn_motion_search", "fdn_motion_residual"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(motion.lib_path()):
        entry.build()
    return motion.lib()


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement, by hand
# ---------------------------------------------------------------------------------------------------------------------------------
def test_candidate_order():
    assert ref.candidates(0) == [(0, 0)]
    assert ref.candidates(1) == [(0, 0), (-1, 0), (0, -1), (0, 1), (1, 0), (-1, -1), (-1, 1), (1, -1), (1, 1)]
    c = ref.candidates(16)
    assert len(c) == 1089 < 2 ** 11 and len(set(c)) == 1089 and c[0] == (0, 0) and c[-1] == (16, 16) and c[-4:-1] == [(-16, -16), (-16, 16), (16, -16)]
    for R in (2, 8):                                                                  # a smaller radius keeps its order among the 1089
        sub = [d for d in c if max(abs(d[0]), abs(d[1])) <= R]
        assert sub == ref.candidates(R)
    assert 256 * 1023 < 2 ** 18


def test_block_grid_and_sums():
    assert ref.block_grid(2, 2) == (1, 1) == motion.block_grid(2, 2) and ref.block_grid(16, 17) == (1, 2) == motion.block_grid(16, 17)
    assert ref.block_grid(720, 1280) == (45, 80) == motion.block_grid(720, 1280) and motion.block_grid(34, 50) == (3, 4)
    a = np.ones((18, 34), dtype=np.int64)
    assert ref.block_sums(a).tolist() == [[256, 256, 32], [32, 32, 4]]                    # the edge blocks hold only their pixels inside


def test_four_by_four_by_hand():
    """cur is prev moved down by one row, the new top row being 9s.  Worked on paper, R = 1, one (partial) block:
         prev rows: 1 2 3 4 / 5 6 7 8 / 9 10 11 12 / 13 14 15 16        cur rows: 9 9 9 9 / 1 2 3 4 / 5 6 7 8 / 9 10 11 12
       d = (-1, 0): cur(y, x) - prev(clamp(y - 1), x): row 0 against prev row 0: |9-1| + |9-2| + |9-3| + |9-4| = 26, rows 1 - 3: 0 -> 26
       d = (0, 0):  row 0: 26; rows 1 - 3: 4 * 4 each = 48 -> 74
       d = (1, 0):  row 0 against prev row 1: 4+3+2+1 = 10; rows 1, 2 against prev rows 2, 3: 8 * 4 = 32 each; row 3 against prev row 3
                    (clamped): 4 * 4 = 16 -> 90
    and every candidate with dx != 0 is worse than (-1, 0): so the vector is (-1, 0), content moved by +1 row, SAD 26, zero-vector SAD 74."""
    prev = np.arange(1, 17, dtype=np.int64).reshape(4, 4)
    cur = np.vstack([np.full((1, 4), 9), prev[:3]])
    assert ref.block_sums(np.abs(cur - ref.shifted(prev, -1, 0))).tolist() == [[26]]
    assert ref.block_sums(np.abs(cur - ref.shifted(prev, 0, 0))).tolist() == [[74]]
    assert ref.block_sums(np.abs(cur - ref.shifted(prev, 1, 0))).tolist() == [[90]]
    assert ref.shifted(prev, -1, 1).tolist() == [[2, 3, 4, 4], [2, 3, 4, 4], [6, 7, 8, 8], [10, 11, 12, 12]]       # the border is replicated
    mv, sad = ref.search_pair(cur, prev, 1)
    assert mv.tolist() == [[[-1, 0]]] and sad.tolist() == [[[26, 74]]]
    frames = ref.frames_of(np.stack([prev, cur]), "yuv420p")
    mvs, sads, stats = ref.search(frames, None, 4, 4, "yuv420p", 1)
    assert mvs.dtype == np.int16 and mvs.tolist() == [[[[0, 0]]], [[[-1, 0]]]] and sads[1].tolist() == [[[26, 74]]]
    assert stats == [(0, 0, 0, 0), (26, 74, 1, 1)]
    # the residual along (-1, 0): rD = cur - prev(clamp(y - 1)) = (8, 7, 6, 5) in row 0, 0 below: 26, 64 + 49 + 36 + 25 = 174; the guide is
    # the stream itself, so words 2 - 3 repeat words 0 - 1 and word 4 is 0
    assert ref.residual(frames, None, frames, None, mvs, 4, 4, "yuv420p") == [(0, 0, 0, 0, 0), (26, 174, 26, 174, 0)]
    # a scored stream that is the guide plus 1 everywhere in frame 1 only: rD = rG + 1: sum |rD| = 26 + 16, sum rD^2 = 81+64+49+36+12 = 242,
    # sum (rD - rG)^2 = 16
    dist = ref.frames_of(np.stack([prev, cur + 1]), "yuv420p")
    assert ref.residual(dist, None, frames, None, mvs, 4, 4, "yuv420p")[1] == (42, 242, 26, 174, 16)
    # with the frame before handed in, a batch that starts at frame 1 says the same
    assert ref.search(frames[1:], frames[0], 4, 4, "yuv420p", 1)[2] == [(26, 74, 1, 1)]
    assert ref.residual(dist[1:], dist[0], frames[1:], frames[0], mvs[1:], 4, 4, "yuv420p") == [(42, 242, 26, 174, 16)]


@pytest.mark.parametrize("pix_fmt", ["yuv420p", "yuv420p10le"])
def test_flat_and_identical_frames(pix_fmt):
    flat = np.full((2, 34, 50), 77, dtype=np.int64)
    mv, sad, stats = ref.search(ref.frames_of(flat, pix_fmt), None, 34, 50, pix_fmt, 8)
    assert not mv.any() and not sad.any() and stats == [(0, 0, 0, 0)] * 2
    one = ref.random_lumas(1, 34, 50, pix_fmt, 5)
    same = ref.frames_of(np.repeat(one, 3, axis=0), pix_fmt)
    mv, sad, stats = ref.search(same, None, 34, 50, pix_fmt, 8)
    assert not mv.any() and not sad.any() and stats == [(0, 0, 0, 0)] * 3
    assert ref.residual(same, None, same, None, mv, 34, 50, pix_fmt) == [(0, 0, 0, 0, 0)] * 3


def test_ten_bit_words_above_the_top_code_count_as_1023():
    y = np.array([[1023, 1024], [65535, 5]])
    assert ref.luma(ref.frames_of(y[None], "yuv420p10le"), 2, 2, "yuv420p10le").tolist() == [[[1023, 1023], [1023, 5]]]


@pytest.mark.parametrize("pix_fmt", ["yuv420p", "yuv420p10le"])
def test_stripes_tie_break(pix_fmt):
    """stripes of period 4: displacements 4 columns apart cost the same, and so does every dy.  The identical frame gives (0, 0) everywhere;
    the frame moved by one column gives (0, -1) in the interior, not (0, 3) or (1, -1)"""
    h, w = 34, 70
    s = ref.stripes(2, h, w, pix_fmt, move=0)
    mv, sad, _ = ref.search(ref.frames_of(s, pix_fmt), None, h, w, pix_fmt, 8)
    assert not mv.any() and not sad.any()
    s = ref.stripes(2, h, w, pix_fmt, move=1)
    mv, sad, _ = ref.search(ref.frames_of(s, pix_fmt), None, h, w, pix_fmt, 8)
    assert (mv[1, :, 1:-1] == (0, -1)).all() and not sad[1, :, 1:-1, 0].any() and sad[1, :, 1:-1, 1].all()
    cur, prev = s[1], s[0]
    assert not np.abs(cur - ref.shifted(prev, 0, 3))[:, 16:48].any() and not np.abs(cur - ref.shifted(prev, 5, -5))[:, 16:48].any()  # the ties


@pytest.mark.parametrize("pix_fmt", ["yuv420p", "yuv420p10le"])
def test_known_shift_is_recovered(pix_fmt):
    """content moving by (-3, +5) per frame: every block whose match lies inside the frame finds (3, -5) with SAD 0"""
    h, w = 70, 130
    s = ref.shifted_stream(3, h, w, pix_fmt, (-3, 5), seed=11)
    mv, sad, stats = ref.search(ref.frames_of(s, pix_fmt), None, h, w, pix_fmt, 8)
    for t in (1, 2):
        assert (mv[t, :-1, 1:] == (3, -5)).all() and not sad[t, :-1, 1:, 0].any() and sad[t, :-1, 1:, 1].all()
        assert stats[t][0] < stats[t][1] and stats[t][3] >= 4 * 8
    r = ref.residual(ref.frames_of(s, pix_fmt), None, ref.frames_of(s, pix_fmt), None, mv, h, w, pix_fmt)
    assert r[1][0] == stats[1][0] and r[1][2:4] == r[1][0:2] and r[1][4] == 0          # sum |rG| along the vectors is the sum of the chosen SADs


# ---------------------------------------------------------------------------------------------------------------------------------
# the library's host side
# ---------------------------------------------------------------------------------------------------------------------------------
def test_version_and_generated_table(lib, monkeypatch):
    spec = importlib.util.spec_from_file_location("gen_abi_table", os.path.join(ROOT, "tools", "gen_abi_table.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    from fdn_hip import _abi_motion as table
    protos, names, members, versions = gen.build_table(headers=["fdn_motion.h"])
    assert table.PROTOTYPES == protos and table.ARG_NAMES == names and list(protos) == members["fdn_motion.h"] == NAMES
    assert table.VERSION == versions["fdn_motion.h"] == ("fdn_motion_abi_version", 1)
    assert "fdn_motion.h" not in gen.HEADERS                                       # the one table of libfdn_hip.so stays what it was
    assert lib.fdn_motion_abi_version() == 1 == motion.ABI_VERSION
    assert lib.fdn_motion_search.argtypes == [ctypes.c_void_p] * 5 + [ctypes.c_int] * 5 + [ctypes.c_void_p]
    assert lib.fdn_motion_residual.argtypes == [ctypes.c_void_p] * 6 + [ctypes.c_int] * 4 + [ctypes.c_void_p]
    assert table.ARG_NAMES["fdn_motion_search"] == ["guide", "guide_prev", "mv", "sad", "stats", "B", "h", "w", "bits", "radius", "stream"]
    assert table.ARG_NAMES["fdn_motion_residual"] == ["frames", "frames_prev", "guide", "guide_prev", "mv", "stats", "B", "h", "w", "bits", "stream"]
    header = open(os.path.join(ROOT, "include", "fdn_motion.h")).read()
    assert f"FDN_MOTION_BLOCK = {motion.BLOCK}, FDN_MOTION_MAX_RADIUS = {motion.MAX_RADIUS}" in header and motion.BLOCK == ref.BLOCK
    import fdn_hip
    from fdn_hip import correct, fusion, sharpness
    for other in (fdn_hip.lib(), correct.lib(), sharpness.lib(), fusion.lib()):    # none of the other libraries holds these entry points
        assert not hasattr(other, "fdn_motion_search") and not hasattr(other, "fdn_motion_residual")
    monkeypatch.setattr(motion, "_lib", None)
    monkeypatch.setattr(motion, "ABI_VERSION", 2)
    with pytest.raises(ImportError, match=r"libfdn_motion\.so has motion ABI version 1, this binding needs 2: rebuild with build\.sh"):
        motion.lib()
    assert motion._lib is None


GOOD = dict(B=2, h=34, w=50, bits=8, radius=8)
BAD = [dict(B=0), dict(B=-1), dict(B=65536), dict(h=33), dict(w=49), dict(h=0), dict(w=0), dict(h=-2), dict(w=-4), dict(h=1), dict(w=1),
       dict(h=32768, w=32768), dict(h=2, w=2 ** 29), dict(bits=9), dict(bits=12), dict(bits=16), dict(bits=0)]


def check_argument_errors(lib):
    """every refusal of include/fdn_motion.h returns FDN_ERR_ARG = 1 before any launch (the pointers are never dereferenced, and a machine
    without a GPU has nothing to launch on)"""
    p = ctypes.c_void_p(64)                                                        # never dereferenced

    def search(ptrs=None, **kw):
        a = {**GOOD, **kw}
        q = dict(guide=p, guide_prev=p, mv=p, sad=p, stats=p)
        q.update(ptrs or {})
        return lib.fdn_motion_search(q["guide"], q["guide_prev"], q["mv"], q["sad"], q["stats"], a["B"], a["h"], a["w"], a["bits"], a["radius"], None)

    def residual(ptrs=None, **kw):
        a = {**GOOD, **kw}
        q = dict(frames=p, frames_prev=p, guide=p, guide_prev=p, mv=p, stats=p)
        q.update(ptrs or {})
        return lib.fdn_motion_residual(q["frames"], q["frames_prev"], q["guide"], q["guide_prev"], q["mv"], q["stats"], a["B"], a["h"], a["w"],
                                       a["bits"], None)

    for bad in BAD:
        assert search(**bad) == 1 and residual(**bad) == 1, bad
    for radius in (-1, 17, 100, -2 ** 31):
        assert search(radius=radius) == 1, radius
    for k in ("guide", "stats"):
        assert search({k: None}) == 1, k
    assert search({"guide": None, "mv": None, "sad": None, "guide_prev": None}) == 1
    for k in ("frames", "guide", "mv", "stats"):
        assert residual({k: None}) == 1, k
    assert residual({"frames_prev": None}) == 1 and residual({"guide_prev": None}) == 1      # exactly one of the two prevs


def test_entry_points_validate_arguments_without_gpu(lib):
    check_argument_errors(lib)


def test_module_refuses_without_a_device(lib):
    from fdn_hip import FdnHipError
    fmt = harness.VideoFormat("yuv420p")
    n = 34 * 50 * 3 // 2
    z = torch.zeros((2, n), dtype=torch.uint8)
    mv = torch.zeros((2, 3, 4, 2), dtype=torch.int16)
    for f in (lambda: motion.search(z, None, 34, 50, fmt), lambda: motion.residual(z, None, z, None, mv, 34, 50, fmt)):
        with pytest.raises(FdnHipError, match="ROCm"):                              # no host fallback
            f()
    with pytest.raises(FdnHipError, match="yuv420p frames must be torch.uint8"):
        motion.search(z.to(torch.int16), None, 34, 50, fmt)
    with pytest.raises(FdnHipError, match=r"expected yuv420p frames \[B, 2550\]"):
        motion.search(z[:, :-1], None, 34, 50, fmt)
    with pytest.raises(FdnHipError, match="the ONE frame before"):
        motion.search(z, z, 34, 50, fmt)
    with pytest.raises(FdnHipError, match="before both streams or before neither"):
        motion.residual(z, z[:1], z, None, mv, 34, 50, fmt)
    for radius in (-1, 17, 2.0, None, True):
        with pytest.raises(ValueError, match="motion radius"):
            motion.search(z, None, 34, 50, fmt, radius=radius)
        with pytest.raises(ValueError, match="motion radius"):
            motion.MotionScore(34, 50, fmt, radius=radius, device="cpu")
    for kw in (dict(h=33), dict(w=49), dict(h=0), dict(h=32768, w=32768)):
        args = dict(h=34, w=50)
        args.update(kw)
        with pytest.raises(ValueError):
            motion.MotionScore(args["h"], args["w"], fmt, device="cpu")
    s = motion.MotionScore(34, 50, fmt, device="cpu")
    with pytest.raises(FdnHipError, match="ROCm"):
        s.update(z)
    assert "flattered" in motion.MotionScore.__doc__                                # what self-compensation hides is said
    src = open(os.path.join(PKG, "fdn_hip", "motion.py")).read()
    assert "oracle" not in src and "tests" not in src.replace("tests/", "")           # the product path stands without the yardsticks


# ---------------------------------------------------------------------------------------------------------------------------------
# MotionScore's host half, on synthetic integers
# ---------------------------------------------------------------------------------------------------------------------------------
def _score(bits=8):
    return motion.MotionScore(34, 50, harness.VideoFormat("yuv420p" if bits == 8 else "yuv420p10le"), device="cpu")


N, NBLK = 34 * 50, 12
SEARCH = [(5, 9, 0, 0), (100, 900, 7, 3), (0, 0, 0, 0), (64, 64, 24, 12), (1, 2, 1, 1)]
RESID = [(9, 9, 9, 9, 9), (300, 1700, 100, 850, 425), (0, 0, 0, 0, 0), (10, 3, 10, 1, 7), (50, 2 ** 40, 50, 2 ** 39, 2 ** 41)]


def test_motion_score_host_logic():
    s = _score()
    assert s.blocks == NBLK and s.frames == [] and s.summary()["frames"] == 0 and math.isnan(s.summary()["mc_psnr_global"])
    s.add_host(SEARCH, RESID, cuts=[True, False, False, True, False])
    f = s.frames
    none = dict.fromkeys(motion.RECORD_KEYS)
    assert f[0] == none and f[3] == none and s.stats[3] == SEARCH[3] + RESID[3]       # at a cut every figure is None, the integers are kept
    assert f[1] == {"mc_psnr": 10 * math.log10(255 * 255 * N / 1700), "mc_psnr_ref": 10 * math.log10(255 * 255 * N / 850),
                    "tc_rmse": math.sqrt(float(Fraction(425, N))), "moving": 0.25, "mean_mv": float(Fraction(7, 12))}
    assert f[1]["tc_rmse"] == 0.5 and f[1]["mc_psnr_ref"] > f[1]["mc_psnr"]
    assert f[2] == {"mc_psnr": math.inf, "mc_psnr_ref": math.inf, "tc_rmse": 0.0, "moving": 0.0, "mean_mv": 0.0}     # inf at zero SSD
    assert f[4]["tc_rmse"] == math.sqrt(float(Fraction(2 ** 41, N))) and f[4]["moving"] == float(Fraction(1, 12))     # exact quotients
    t = s.summary()
    assert t["frames"] == 5 and t["cuts"] == 2 and t["mc_psnr"] == math.inf
    assert t["tc_rmse"] == math.fsum([0.5, 0.0, f[4]["tc_rmse"]]) / 3 and t["moving"] == math.fsum([0.25, 0.0, f[4]["moving"]]) / 3
    assert t["mc_psnr_global"] == 10 * math.log10(255 * 255 * 3 * N / (1700 + 2 ** 40))
    assert t["mc_psnr_ref_global"] == 10 * math.log10(255 * 255 * 3 * N / (850 + 2 ** 39))
    assert t["tc_rmse_global"] == math.sqrt(float(Fraction(425 + 2 ** 41, 3 * N)))
    # the stream's first frame is a cut whatever the flags say; cuts=None: only that one
    s = _score()
    s.add_host(SEARCH[:2], RESID[:2], cuts=[False, False])
    assert s.frames[0] == none and s.frames[1] == f[1]
    s = _score()
    s.add_host(SEARCH, RESID)
    assert [r["mc_psnr"] is None for r in s.frames] == [True, False, False, False, False]


def test_motion_score_batches_and_bit_depth():
    cuts = [True, False, False, True, False]
    whole = _score()
    whole.add_host(SEARCH, RESID, cuts)
    for split in ([1, 1, 1, 1, 1], [3, 2], [1, 4]):
        s, at = _score(), 0
        for k in split:
            s.add_host(SEARCH[at:at + k], RESID[at:at + k], cuts[at:at + k])
            at += k
        assert s.frames == whole.frames and s.stats == whole.stats
        a, b = s.summary(), whole.summary()
        assert a.keys() == b.keys() and all(a[k] == b[k] or (math.isnan(a[k]) and math.isnan(b[k])) for k in a)
    # 10 bit: the peak is 1023 and tc_rmse is brought to 8-bit code units: the same stream at four times the codes scores the same tc
    s10 = _score(10)
    s10.add_host(SEARCH, [(4 * r[0], 16 * r[1], 4 * r[2], 16 * r[3], 16 * r[4]) for r in RESID], cuts)
    assert s10.frames[1]["tc_rmse"] == 0.5 == whole.frames[1]["tc_rmse"]
    assert s10.frames[1]["mc_psnr"] == 10 * math.log10(1023 * 1023 * N / (16 * 1700))
    # without a reference there is no truth: mc_psnr_ref and tc_rmse stay None, their pooled figures nan
    s = _score()
    s.add_host(SEARCH, RESID, cuts, has_ref=False)
    assert s.frames[1]["mc_psnr"] == whole.frames[1]["mc_psnr"] and s.frames[1]["mc_psnr_ref"] is None and s.frames[1]["tc_rmse"] is None
    t = s.summary()
    assert math.isnan(t["tc_rmse"]) and math.isnan(t["mc_psnr_ref_global"]) and math.isnan(t["tc_rmse_global"]) and t["moving"] == whole.summary()["moving"]
    with pytest.raises(ValueError, match="on every call or on none"):
        s.add_host(SEARCH[:1], RESID[:1], [False])
    # an all-cut stream: nothing to average
    s = _score()
    s.add_host(SEARCH, RESID, cuts=[True] * 5)
    t = s.summary()
    assert t["frames"] == 5 and t["cuts"] == 5 and all(math.isnan(t[k]) for k in t if k not in ("frames", "cuts"))


def test_restated_records_agree_with_add_host():
    """motion_ref.records, the yardstick of the GPU test, against MotionScore.add_host fed the restatement's integers"""
    pix = "yuv420p10le"
    h, w = 34, 50
    g = ref.shifted_stream(5, h, w, pix, (1, -2), seed=3)
    d = np.clip(g + np.random.default_rng(4).integers(-6, 7, size=g.shape), 0, 1023)
    gf, df = ref.frames_of(g, pix), ref.frames_of(d, pix)
    cuts = [True, False, True, False, False]
    recs, summary = ref.records(df, gf, h, w, pix, R=4, cuts=cuts)
    mv, _, ss = ref.search(gf, None, h, w, pix, 4)
    s = motion.MotionScore(h, w, harness.VideoFormat(pix), radius=4, device="cpu")
    s.add_host(ss, ref.residual(df, None, gf, None, mv, h, w, pix), cuts)
    assert s.frames == recs and recs[1]["tc_rmse"] > 0 and recs[2]["mc_psnr"] is None
    t = s.summary()
    assert t.keys() == summary.keys() and all(t[k] == summary[k] for k in t)


# ---------------------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------------------
def test_command_line(monkeypatch, capsys):
    sys.path.insert(0, PKG)
    import calculate_video_metrics as tool

    def touched(*a, **k):
        raise AssertionError("the tool touched the device")
    monkeypatch.setattr(torch.cuda, "set_device", touched)
    monkeypatch.setattr(torch.cuda, "is_available", touched)
    a = tool.parse_args(["--ref", "a.y4m", "b.y4m"])
    assert a.motion is False and a.motion_radius == 8
    a = tool.parse_args(["--ref", "a.y4m", "b.y4m", "--motion"])
    assert a.motion is True and a.motion_radius == 8
    for n in (0, 1, 16):
        assert tool.parse_args(["b.y4m", "--motion", "--motion-radius", str(n)]).motion_radius == n
    for argv in (["b.y4m", "--motion-radius", "4"], ["b.y4m", "--motion-radius", "8"], ["b.y4m", "--motion", "--motion-radius", "17"],
                 ["b.y4m", "--motion", "--motion-radius", "-1"], ["b.y4m", "--motion", "--motion-radius", "2.5"],
                 ["b.y4m", "--motion", "--motion-radius"]):
        with pytest.raises(SystemExit):
            tool.parse_args(argv)
        assert "--motion" in capsys.readouterr().err
    assert tool.CSV_COLUMNS == ("frame", "psnr_y", "psnr_u", "psnr_v", "psnr_avg", "ssim_y", "mean_y_ref", "mean_y", "cut", "dmean_ref", "dmean")
    assert tool.MOTION_COLUMNS == motion.RECORD_KEYS
    m = {"mc_psnr": 31.25, "mc_psnr_ref": math.inf, "tc_rmse": 0.5, "moving": 0.25, "mean_mv": 1.5}
    assert tool.motion_part(m, True) == ", mc-PSNR 31.2500 (ref inf), tc 0.5000, moving 0.250"
    assert tool.motion_part(m, False) == ", mc-PSNR 31.2500, moving 0.250"
    assert tool.motion_part(dict.fromkeys(motion.RECORD_KEYS), True) == ", mc-PSNR - (ref -), tc -, moving -"
    assert tool.motion_cells(m) == "31.25,inf,0.5,0.25,1.5" and tool.motion_cells(dict.fromkeys(motion.RECORD_KEYS)) == ",,,,"
