"""CPU: the host side of video evaluation - the entry points of include/fdn_vmetrics.h (version, prototype table, argument checks before
any launch), the restatement of tests/vmetrics_ref.py judged on its own (its SSIM against the oracle's _ssim_planes, its integers by
hand), the host arithmetic of fdn_hip.video_metrics and of VideoScore on synthetic integer sums and histograms, and what
calculate_video_metrics.py refuses before it touches a device.  No GPU compute."""
import ctypes
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

import __graft_entry__ as entry  # noqa: F401  (puts the package on sys.path)
import vmetrics_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fdn-tip2025_amd")
NAMES = ["fdn_vmetrics_abi_version", "fdn_yuv420_pair_stats", "fdn_yuv420_ssim_y_ws", "fdn_yuv420_ssim_y"]


@pytest.fixture(scope="module")
def lib():
    import fdn_hip
    if not os.path.isfile(fdn_hip.lib_path()):
        entry.build()
    return fdn_hip.lib()


def test_versions_and_prototype_table(lib):
    """the entry points of include/fdn_vmetrics.h in the one table (tests/test_host_cpu.py holds it to the headers): names, signatures"""
    from fdn_hip._abi import HEADERS, PROTOTYPES
    assert HEADERS["fdn_vmetrics.h"] == NAMES
    assert PROTOTYPES["fdn_yuv420_pair_stats"] == ("I", ["P", "P", "P", "I", "I", "I", "I", "I", "P"])
    assert PROTOTYPES["fdn_yuv420_ssim_y_ws"] == ("L", ["I", "I", "I"])
    assert PROTOTYPES["fdn_yuv420_ssim_y"] == ("I", ["P", "P", "P", "P", "P", "I", "I", "I", "I", "P"])
    assert lib.fdn_yuv420_ssim_y_ws.restype == ctypes.c_long and lib.fdn_yuv420_ssim_y_ws.argtypes == [ctypes.c_int] * 3
    assert lib.fdn_yuv420_pair_stats.argtypes == [ctypes.c_void_p] * 3 + [ctypes.c_int] * 5 + [ctypes.c_void_p]


BAD_SIZES = [dict(h=33), dict(w=37), dict(h=0), dict(w=0), dict(h=-2), dict(w=-2), dict(h=1, w=1), dict(h=32768, w=32768),
             dict(h=65536, w=65536), dict(h=2, w=2 ** 30)]
BAD_B = [dict(B=0), dict(B=-1), dict(B=65536)]


def test_entry_points_validate_arguments_without_gpu(lib):
    """every refusal of include/fdn_vmetrics.h returns FDN_ERR_ARG = 1 before any launch; the workspace query answers 0 to the same sizes"""
    p = ctypes.c_void_p(64)                          # never dereferenced: every call below fails its argument check
    taps = (ctypes.c_double * 11)(*ref.taps())

    def stats(a=p, b=p, out=p, B=1, h=34, w=38, layout=0, bits=8):
        return lib.fdn_yuv420_pair_stats(a, b, out, B, h, w, layout, bits, None)

    def ssim(a=p, b=p, out=p, ws=p, taps=ctypes.cast(taps, ctypes.c_void_p), B=1, h=34, w=38, bits=8):
        return lib.fdn_yuv420_ssim_y(a, b, out, ws, taps, B, h, w, bits, None)

    assert stats(a=None) == 1 and stats(out=None) == 1 and stats(a=None, b=None) == 1          # b alone may be NULL
    for key in ("a", "b", "out", "ws", "taps"):
        assert ssim(**{key: None}) == 1, key
    for kw in BAD_B + BAD_SIZES + [dict(bits=9), dict(bits=12), dict(bits=16), dict(bits=0)]:
        assert stats(**kw) == 1, kw
        assert ssim(**kw) == 1, kw
    assert stats(layout=1, bits=10) == 1 and stats(layout=2) == 1 and stats(layout=-1) == 1
    for kw in BAD_B + BAD_SIZES:
        args = dict(B=1, h=34, w=38)
        args.update(kw)
        assert lib.fdn_yuv420_ssim_y_ws(args["B"], args["h"], args["w"]) == 0, kw
    assert lib.fdn_yuv420_ssim_y_ws(1, 2, 2) == 1 and lib.fdn_yuv420_ssim_y_ws(3, 2, 2) == 3
    n = lib.fdn_yuv420_ssim_y_ws(2, 70, 514)
    assert n > 0 and n % 2 == 0 and lib.fdn_yuv420_ssim_y_ws(1, 70, 514) == n // 2
    assert lib.fdn_yuv420_ssim_y_ws(65535, 1080, 1920) > 0 and lib.fdn_yuv420_ssim_y_ws(1, 2, 2 ** 29 - 2) > 0


def _plane_pairs(rng, h, w, bits):
    top = 2 ** bits - 1
    a = rng.integers(0, top + 1, size=(h, w))
    yield "random", a, rng.integers(0, top + 1, size=(h, w))
    yield "near", a, np.clip(a + rng.integers(-2, 3, size=(h, w)), 0, top)
    yield "identical", a, a
    yield "flat", np.full((h, w), 17 * 2 ** (bits - 8)), np.full((h, w), 203 * 2 ** (bits - 8))


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("shape", [(2, 2), (12, 14), (34, 38), (70, 514)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_ssim_against_the_oracle(shape, bits):
    """the separable float64 restatement against the oracle's 11 x 11 window (_ssim_planes, replicate border, whole map), within 1e-12:
    two float64 summation orders of the same map differ by at most 3.7e-13 (measured on the CPU, the largest on the flat pair)"""
    import fdn_oracle as O
    h, w = shape
    rng = np.random.default_rng(100 * h + bits)
    L = 2 ** bits - 1
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    for name, a, b in _plane_pairs(rng, h, w, bits):
        want = float(O._ssim_planes(torch.from_numpy(a).to(torch.float64), torch.from_numpy(b).to(torch.float64), C1, C2, "replicate", False).mean())
        got = ref.ssim_plane(a, b, bits)
        print(f"{h}x{w} {bits} bit {name}: {got!r} oracle {want!r} diff {abs(got - want):.3e}")
        assert abs(got - want) <= 1e-12, name
        if name == "identical":
            assert abs(got - 1.0) <= 1e-12
    assert np.array_equal(ref.taps(), O.gaussian_kernel_11().numpy())
    from fdn_hip import metrics
    assert np.array_equal(ref.taps(), metrics.ssim3d_taps())


def test_hand_checked_integers():
    from fdn_hip import video_metrics as vm
    # a 2 x 2 frame: luma differences 1, 2, 3, 4, Cb 5, Cr 6
    a = np.array([[10, 20, 30, 40, 100, 200]], dtype=np.uint8)
    b = np.array([[11, 18, 33, 36, 105, 194]], dtype=np.uint8)
    assert ref.pair_stats(a, b, 2, 2, "yuv420p") == [(1 + 4 + 9 + 16, 25, 36, 100, 98)]
    assert ref.pair_stats(a, b, 2, 2, "nv12") == [(30, 25, 36, 100, 98)]                        # one chroma pair: the same bytes
    assert ref.pair_stats(a, None, 2, 2, "yuv420p") == [(0, 0, 0, 100, 0)]
    # 10 bit: words above 1023 count as 1023
    a10 = np.array([[0, 1023, 1024, 65535, 0, 2000]], dtype=np.uint16)
    b10 = np.array([[0, 1023, 1023, 1023, 1023, 1023]], dtype=np.uint16)
    assert ref.pair_stats(a10, b10, 2, 2, "yuv420p10le") == [(0, 1023 ** 2, 0, 3 * 1023, 3 * 1023)]
    # all 0 against all 1023
    h, w = 70, 514
    zero, full = np.zeros((1, h * w * 3 // 2), dtype=np.uint16), np.full((1, h * w * 3 // 2), 1023, dtype=np.uint16)
    st = ref.pair_stats(zero, full, h, w, "yuv420p10le")[0]
    assert st == (1023 ** 2 * h * w, 1023 ** 2 * h * w // 4, 1023 ** 2 * h * w // 4, 0, 1023 * h * w) and st[0] > 2 ** 32
    assert vm.psnr_from_sse(st[0], h * w, 10) == 0.0 and vm.psnr_avg(st[0], st[1], st[2], h, w, 10) == 0.0
    # PSNR
    assert vm.psnr_from_sse(0, 4, 8) == float("inf") and vm.psnr_from_sse(0, 4, 10) == float("inf")
    assert vm.psnr_from_sse(4, 4, 8) == 10.0 * math.log10(255.0 ** 2) and vm.psnr_from_sse(30, 4, 8) == 10.0 * math.log10(255 * 255 * 4 / 30)
    assert vm.psnr_from_sse(30, 4, 8) == ref.psnr(30, 4, 8)
    assert vm.psnr_avg(30, 25, 36, 2, 2, 8) == 10.0 * math.log10(255 * 255 * 6 / 91)           # pooled over h w 3 / 2 = 6 samples
    assert vm.psnr_avg(6, 0, 0, 2, 2, 8) == vm.psnr_from_sse(4, 4, 8)
    assert vm.psnr_avg(0, 0, 0, 2, 2, 10) == float("inf")
    # cut_above is RatioFilter's
    from fdn_hip.temporal import RatioFilter
    for h, w, cut in ((34, 38, 0.3), (720, 1280, 0.7), (2, 2, 0.99), (34, 38, 0.0), (34, 38, 1.0)):
        assert vm.cut_above(cut, h, w) == RatioFilter(h, w, 8, 1.0, cut=cut, device="cpu").cut_above == ref.cut_above(cut, h, w)
    assert vm.cut_above(0.3, 34, 38) == 775
    # dmean: exact, in 8-bit code units
    assert vm.dmean(1292 * 3, 1292, 34, 38, 8) == 2.0 and vm.dmean(1292 * 3, 1292, 34, 38, 10) == 0.5
    assert vm.dmean(1, 0, 34, 38, 8) == float(Fraction(1, 1292)) and vm.dmean(0, 7, 34, 38, 10) == float(Fraction(-7, 5168))
    assert vm.mean_luma(1292 * 1023, 34, 38, 10) == 255.75


def _hist(bins):
    out = [0] * 256
    for k, v in bins.items():
        out[k] = v
    return out


def _score(device="cpu", bits=8, cut=0.3):
    from fdn_hip import harness
    from fdn_hip.video_metrics import VideoScore
    return VideoScore(34, 38, harness.VideoFormat("yuv420p" if bits == 8 else "yuv420p10le"), cut=cut, device=device)


def test_video_score_host_logic():
    """synthetic integers through VideoScore.add_host: the first frame is a cut, the threshold is `>`, dmean skips cuts, the three
    flicker figures, nan where there is nothing to average; fed whole and frame by frame"""
    n = 34 * 38                                                                          # 1292, cut_above 775
    s = _score()
    assert s.cut_above == 775 and s.frames == [] and s.summary()["frames"] == 0
    empty = s.summary()
    assert all(math.isnan(empty[k]) for k in ("psnr_y", "ssim_y", "mean_y", "flicker", "flicker_ref", "flicker_err", "psnr_avg_global"))
    assert empty["cuts"] == 0
    base = {10: n}
    from fdn_hip.video_metrics import hist_distance
    # frames: 0 first; 1 same histogram; 2 at distance 774 (no cut); 3 at distance 776 from frame 2 (cut); 4 same as 3
    hists = [_hist(base), _hist(base), _hist({10: n - 387, 11: 387}), _hist({10: n - 387 - 388, 11: 387, 12: 388}), None]
    hists[4] = hists[3]
    assert hist_distance(hists[2], hists[1]) == 774 and hist_distance(hists[3], hists[2]) == 776 and hist_distance(hists[4], hists[3]) == 0
    sums_d = [1000, 1000 + n, 1000 + 3 * n, 9000, 9000 - n // 2]
    sums_r = [2000, 2000, 2000 + n, 8000, 8000 + n]
    stats = [(4 * t, t, 0, sums_d[t], sums_r[t]) for t in range(5)]
    ssim = [1.0, 0.9, 0.8, 0.7, 0.6]
    s.add_host(stats, hists, ssim)
    f = s.frames
    assert [r["cut"] for r in f] == [True, False, False, True, False]
    assert [r["dmean"] for r in f] == [None, 1.0, 2.0, None, -0.5]
    assert [r["dmean_ref"] for r in f] == [None, 0.0, 1.0, None, 1.0]
    assert f[0]["psnr_y"] == float("inf") and f[0]["psnr_v"] == float("inf") and f[1]["psnr_y"] == 10 * math.log10(255 * 255 * n / 4)
    assert f[1]["psnr_u"] == 10 * math.log10(255 * 255 * (n // 4) / 1) and f[1]["psnr_avg"] == 10 * math.log10(255 * 255 * (n * 3 // 2) / 5)
    assert [r["ssim_y"] for r in f] == ssim and f[1]["mean_y"] == float(Fraction(1000 + n, n)) and f[1]["mean_y_ref"] == float(Fraction(2000, n))
    assert s.stats == stats
    out = s.summary()
    assert out["frames"] == 5 and out["cuts"] == 2
    assert out["flicker"] == (1.0 + 2.0 + 0.5) / 3 and out["flicker_ref"] == 2.0 / 3 and out["flicker_err"] == (1.0 + 1.0 + 1.5) / 3
    assert out["ssim_y"] == math.fsum(ssim) / 5 and out["psnr_y"] == float("inf")
    assert out["psnr_y_global"] == 10 * math.log10(255 * 255 * 5 * n / 40) and out["psnr_v_global"] == float("inf")
    assert out["psnr_avg_global"] == 10 * math.log10(255 * 255 * 5 * (n * 3 // 2) / 50)
    # the edge of the threshold, on histograms the host logic takes as they come: dist == cut_above is no cut, cut_above + 1 is one
    for drop, flag in ((775, False), (776, True), (0, False)):
        e = _score()
        e.add_host([(0, 0, 0, 1, 1)] * 2, [_hist(base), _hist({10: n - drop})], [1.0, 1.0])
        assert hist_distance(_hist(base), _hist({10: n - drop})) == drop and [r["cut"] for r in e.frames] == [True, flag]
    # batching does not matter
    one = _score()
    for t in range(5):
        one.add_host(stats[t:t + 1], hists[t:t + 1], ssim[t:t + 1])
    three = _score()
    three.add_host(stats[:3], hists[:3], ssim[:3])
    three.add_host(stats[3:], hists[3:], ssim[3:])
    assert one.frames == f and three.frames == f and one.summary() == out and three.summary() == out
    # without a reference: no PSNR, no SSIM, no *_ref; flicker alone
    alone = _score()
    alone.add_host([(0, 0, 0, sums_d[t], 0) for t in range(5)], hists)
    assert [r["dmean"] for r in alone.frames] == [None, 1.0, 2.0, None, -0.5]
    assert all(r["psnr_y"] is None and r["ssim_y"] is None and r["mean_y_ref"] is None and r["dmean_ref"] is None for r in alone.frames)
    o = alone.summary()
    assert o["flicker"] == out["flicker"] and math.isnan(o["flicker_ref"]) and math.isnan(o["flicker_err"]) and math.isnan(o["psnr_y"])
    assert math.isnan(o["psnr_y_global"]) and o["mean_y"] == out["mean_y"]
    with pytest.raises(ValueError, match="reference"):
        alone.add_host(stats[:1], hists[:1], ssim[:1])
    # every frame a cut: nothing to average
    cuts = _score(cut=0.0)
    cuts.add_host([(0, 0, 0, 5, 5)] * 2, [_hist(base), _hist({11: n})], [1.0, 1.0])
    assert [r["cut"] for r in cuts.frames] == [True, True] and math.isnan(cuts.summary()["flicker"]) and cuts.summary()["cuts"] == 2
    # the restatement's flicker figures are the module's
    recs = [dict(r) for r in f]
    assert ref.flicker(recs) == (out["flicker"], out["flicker_ref"], out["flicker_err"])


def test_video_score_checks_its_arguments():
    from fdn_hip import FdnHipError, harness
    from fdn_hip import video_metrics as vm
    fmt = harness.VideoFormat("yuv420p")
    for kw in (dict(h=33), dict(w=37), dict(h=0), dict(h=32768, w=32768), dict(cut=-0.1), dict(cut=1.1), dict(cut=float("nan"))):
        args = dict(h=34, w=38, cut=0.3)
        args.update(kw)
        with pytest.raises(ValueError):
            vm.VideoScore(args["h"], args["w"], fmt, cut=args["cut"], device="cpu")
    s = vm.VideoScore(34, 38, fmt, device="cpu")
    n = 34 * 38 * 3 // 2
    with pytest.raises(FdnHipError, match="ROCm"):                                       # no host fallback
        s.update(torch.zeros(2, n, dtype=torch.uint8))
    with pytest.raises(FdnHipError, match="frames must be"):
        s.update(torch.zeros(2, n, dtype=torch.int16))
    with pytest.raises(FdnHipError, match="expected"):
        s.update(torch.zeros(2, n - 1, dtype=torch.uint8))
    with pytest.raises(FdnHipError, match="differ"):
        vm.pair_stats(torch.zeros(2, n, dtype=torch.uint8), torch.zeros(3, n, dtype=torch.uint8), 34, 38, fmt)
    with pytest.raises(FdnHipError, match="ROCm"):
        vm.ssim_y(torch.zeros(2, n, dtype=torch.uint8), torch.zeros(2, n, dtype=torch.uint8), 34, 38, fmt)
    assert s.frames == []


def _y4m(path, w, h, tag, frames):
    with open(path, "wb") as f:
        f.write(f"YUV4MPEG2 W{w} H{h} F25:1 Ip A1:1 C{tag}\n".encode())
        for fr in frames:
            f.write(b"FRAME\n" + fr.tobytes())
    return str(path)


def test_tool_refuses_before_touching_a_device(tmp_path, monkeypatch):
    """mismatched sizes or pix_fmt and a --size that contradicts the header: SystemExit with one line, before torch is asked for a device"""
    import calculate_video_metrics as tool

    def touched(*a, **k):
        raise AssertionError("the tool touched the device")
    monkeypatch.setattr(torch.cuda, "set_device", touched)
    monkeypatch.setattr(torch.cuda, "is_available", touched)
    f8 = ref.random_frames(1, 2, 34, 38, "yuv420p")
    a = _y4m(tmp_path / "a.y4m", 38, 34, "420mpeg2", f8)
    b = _y4m(tmp_path / "b.y4m", 38, 36, "420mpeg2", ref.random_frames(2, 2, 36, 38, "yuv420p"))
    c = _y4m(tmp_path / "c.y4m", 38, 34, "420p10", ref.random_frames(3, 2, 34, 38, "yuv420p10le"))
    raw = str(tmp_path / "d.yuv")
    f8.tofile(raw)
    cases = [(["--ref", a, b], "differ in size"), (["--ref", a, c], "differ in pix_fmt"), (["--ref", a, a, "--size", "40x34"], "contradicts"),
             ([a, "--size", "40x34"], "contradicts"), ([raw], "needs --size"), (["--ref", a, str(tmp_path / "none.y4m")], "none.y4m"),
             (["--ref", a, raw, "--size", "38x36"], "contradicts"), (["--ref", raw, c, "--size", "38x34"], "differ in pix_fmt")]
    for argv, word in cases:
        with pytest.raises(SystemExit) as e:
            tool.main(argv)
        msg = str(e.value.code)
        assert msg.startswith("calculate_video_metrics.py: ") and word in msg and "\n" not in msg, (argv, msg)
    for argv in (["--batch", "0", a], ["--scene-cut", "1.5", a], ["--ref", "-", a], []):
        with pytest.raises(SystemExit):
            tool.parse_args(argv)
    ok = tool.parse_args(["--ref", a, "-"])
    assert (ok.ref, ok.dist, ok.batch, ok.scene_cut, ok.csv, ok.device, ok.format) == (a, "-", 8, 0.3, None, "cuda:0", "auto")
    # and as a process: one line on stderr, nothing on stdout, no traceback
    run = subprocess.run([sys.executable, os.path.join(PKG, "calculate_video_metrics.py"), "--ref", a, b], capture_output=True, timeout=300)
    err = run.stderr.decode()
    assert run.returncode != 0 and run.stdout == b"" and "Traceback" not in err and len(err.strip().split("\n")) == 1 and "differ in size" in err
