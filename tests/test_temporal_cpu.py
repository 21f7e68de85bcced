"""CPU: the host side of the ratio filter across frames - the entry points of include/fdn_temporal.h (version, prototype table, argument
checks before any launch), the restatement of tests/temporal_ref.py judged on its own, the checks fdn_hip.temporal.RatioFilter and
fdn_hip.harness.enhance_yuv420(temporal=...) make before anything runs, and the two flags of inference_fdn_video.py.  No GPU compute."""
import ctypes
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as entry  # noqa: F401  (puts the package on sys.path)
import temporal_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fdn_temporal_abi_version", "fdn_luma_hist", "fdn_ratio_smooth"]


@pytest.fixture(scope="module")
def lib():
    import fdn_hip
    if not os.path.isfile(fdn_hip.lib_path()):
        entry.build()
    return fdn_hip.lib()


def test_version_and_prototype_table(lib):
    """the entry points of include/fdn_temporal.h in the one table (tests/test_host_cpu.py holds it to the headers): names, signatures"""
    from fdn_hip._abi import HEADERS, PROTOTYPES
    header = os.path.join(ROOT, "include", "fdn_temporal.h")
    assert HEADERS["fdn_temporal.h"] == NAMES
    assert PROTOTYPES["fdn_luma_hist"] == ("I", ["P", "P", "I", "I", "I", "I", "P"])
    assert PROTOTYPES["fdn_ratio_smooth"] == ("I", ["P", "P", "P", "F", "I", "I", "P", "P", "P", "P"])
    assert lib.fdn_ratio_smooth.argtypes == [ctypes.c_void_p] * 3 + [ctypes.c_float, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 4
    assert "#define FDN_TEMPORAL_STATE_WORDS 258" in open(header).read()
    from fdn_hip import temporal
    assert temporal.STATE_WORDS == ref.STATE_WORDS == 258


def test_entry_points_validate_arguments_without_gpu(lib):
    """every refusal of include/fdn_temporal.h returns FDN_ERR_ARG = 1 before any launch"""
    p = ctypes.c_void_p(64)                          # never dereferenced: every call below fails its argument check

    def hist(frames=p, out=p, B=1, h=34, w=38, bits=8):
        return lib.fdn_luma_hist(frames, out, B, h, w, bits, None)
    assert hist(frames=None) == 1 and hist(out=None) == 1
    assert hist(B=0) == 1 and hist(B=-1) == 1 and hist(B=65536) == 1
    assert hist(h=33) == 1 and hist(w=37) == 1 and hist(h=0) == 1 and hist(w=0) == 1 and hist(h=-2) == 1 and hist(w=-2) == 1
    assert hist(bits=9) == 1 and hist(bits=12) == 1 and hist(bits=16) == 1 and hist(bits=0) == 1
    assert hist(h=32768, w=32768) == 1 and hist(h=65536, w=65536) == 1 and hist(h=2, w=2 ** 30) == 1     # h w >= 2^30

    def smooth(hist=p, ratio=p, state=p, alpha=0.5, cut_above=10, B=1, out=p, dist=p, cut=p):
        return lib.fdn_ratio_smooth(hist, ratio, state, alpha, cut_above, B, out, dist, cut, None)
    for key in ("hist", "ratio", "state", "out", "dist", "cut"):
        assert smooth(**{key: None}) == 1, key
    assert smooth(B=0) == 1 and smooth(B=-3) == 1 and smooth(B=65536) == 1
    for alpha in (0.0, -0.25, 1.0000001, 2.0, float("nan"), float("inf")):
        assert smooth(alpha=alpha) == 1, alpha
    assert smooth(cut_above=-1) == 1 and smooth(cut_above=-2 ** 31) == 1


def test_restatement_histogram():
    """bin = code >> (bits - 8), a 10-bit word above 1023 counts as 1023, chroma is never counted, every row sums to h w"""
    y8 = np.array([[0, 1, 255, 255, 9, 9]], dtype=np.uint8)                        # 2 x 2: four luma samples, two of chroma
    h8 = ref.luma_hist(y8, 2, 2, 8)
    assert h8.dtype == np.uint32 and h8.shape == (1, 256) and h8.sum() == 4
    assert h8[0, 0] == 1 and h8[0, 1] == 1 and h8[0, 255] == 2 and h8[0, 9] == 0
    y10 = np.array([[3, 4, 1023, 1024, 7, 7], [65535, 1020, 1019, 0, 7, 7]], dtype=np.uint16)
    h10 = ref.luma_hist(y10, 2, 2, 10)
    assert list(h10.sum(axis=1)) == [4, 4]
    assert h10[0, 0] == 1 and h10[0, 1] == 1 and h10[0, 255] == 2 and h10[1, 255] == 2 and h10[1, 254] == 1 and h10[1, 0] == 1


def _hists(rng, B, total=2000, bins=(0, 100)):
    """B histograms over a range of bins, each summing to `total`"""
    out = np.zeros((B, 256), dtype=np.uint32)
    for t in range(B):
        out[t] = np.bincount(rng.integers(bins[0], bins[1], size=total), minlength=256)
    return out


def test_restatement_constant_ratio_and_step_response():
    rng = np.random.default_rng(1)
    hist = _hists(rng, 6)
    big = 2 * 2000                                                                  # no cut but the first frame
    r = np.full(6, 0.3, dtype=np.float32)
    out, dist, cut, state = ref.smooth(hist, r, ref.zero_state(), 0.25, big)
    assert np.array_equal(out, r) and list(cut) == [1, 0, 0, 0, 0, 0] and dist[0] == 0 and np.all(dist[1:] > 0)
    assert state[257] == 3 and state[256] == r.view(np.uint32)[0] and np.array_equal(state[:256], hist[-1])
    # a step from 0.2 to 0.6: out[t] = prev + alpha * (r - prev), each operation rounded to float32
    r = np.array([0.2, 0.6, 0.6, 0.6], dtype=np.float32)
    alpha = np.float32(0.25)
    out = ref.smooth(hist[:4], r, ref.zero_state(), 0.25, big)[0]
    prev = np.float32(0.2)
    assert out[0] == prev
    for t in range(1, 4):
        want = np.float32(prev + np.float32(alpha * np.float32(r[t] - prev)))
        assert out[t] == want and prev < out[t] < r[t]
        prev = want
    assert abs(float(out[1]) - 0.3) < 1e-6 and abs(float(out[2]) - 0.375) < 1e-6
    # distances are plain L1 distances
    assert dist[1] == np.abs(hist[1].astype(np.int64) - hist[0].astype(np.int64)).sum()


def test_restatement_cut_resets_and_alpha_one_is_identity():
    rng = np.random.default_rng(2)
    hist = np.concatenate([_hists(rng, 3, bins=(0, 100)), _hists(rng, 3, bins=(150, 250))])
    r = rng.uniform(0.05, 0.6, size=6).astype(np.float32)
    out, dist, cut, _ = ref.smooth(hist, r, ref.zero_state(), 0.25, 1200)         # 0.3 of 2 x 2000
    assert list(cut) == [1, 0, 0, 1, 0, 0] and dist[3] == 4000 and np.all(dist[[1, 2, 4, 5]] <= 1200)
    assert out[0] == r[0] and out[3] == r[3]                                        # a cut hands the frame's own ratio out
    assert out[1] != r[1] and out[4] != r[4]
    assert out[4] == np.float32(r[3] + np.float32(np.float32(0.25) * np.float32(r[4] - r[3])))   # and the filter goes on from it
    # the edge of the threshold: equal is no cut, one more is
    d = int(dist[1])
    assert ref.smooth(hist[:2], r[:2], ref.zero_state(), 0.25, d)[2][1] == 0
    assert ref.smooth(hist[:2], r[:2], ref.zero_state(), 0.25, d - 1)[2][1] == 1
    # alpha = 1 hands every ratio out as it is, even where prev + (r - prev) would not round back to r, and still finds the cuts
    wild = np.array([1.0, 0.3, 1e-10, 7.0, 0.1, 0.3], dtype=np.float32)
    assert np.float32(np.float32(1.0) + np.float32(wild[2] - np.float32(1.0))) != wild[2]
    out1, _, cut1, state1 = ref.smooth(hist, wild, ref.zero_state(), 1.0, 1200)
    assert np.array_equal(out1.view(np.uint32), wild.view(np.uint32)) and list(cut1) == [1, 0, 0, 1, 0, 0]
    assert state1[256] == wild.view(np.uint32)[-1]


def test_restatement_nan_passes_and_does_not_poison():
    rng = np.random.default_rng(3)
    hist = _hists(rng, 5)
    for bad in (np.nan, np.inf, -np.inf):
        r = np.array([0.2, 0.4, bad, 0.4, 0.4], dtype=np.float32)
        out, _, cut, state = ref.smooth(hist, r, ref.zero_state(), 0.5, 4000)
        assert list(cut) == [1, 0, 0, 0, 0]
        assert out[2].view(np.uint32) == r[2].view(np.uint32)                      # handed out as it is
        assert np.all(np.isfinite(out[[0, 1, 3, 4]]))
        clean = ref.smooth(hist[[0, 1, 3, 4]], r[[0, 1, 3, 4]], ref.zero_state(), 0.5, 4000)[0]
        assert np.array_equal(out[[0, 1, 3, 4]], clean)                            # frame 3 filters against frame 1's value
        assert state[257] == 3 and np.isfinite(state[256:257].view(np.float32)[0])
    # a stream that starts with NaN has no ratio until the first finite one, which is then handed out unfiltered
    r = np.array([np.nan, 0.4, 0.2], dtype=np.float32)
    out, _, _, state = ref.smooth(hist[:3], r, ref.zero_state(), 0.5, 4000)
    assert np.isnan(out[0]) and out[1] == np.float32(0.4) and out[2] == np.float32(0.4) + np.float32(0.5) * (np.float32(0.2) - np.float32(0.4))
    only_nan = ref.smooth(hist[:1], r[:1], ref.zero_state(), 0.5, 4000)[3]
    assert only_nan[257] == 1 and only_nan[256] == 0                               # has a frame, has no ratio
    # the histogram advances on a NaN frame too
    assert np.array_equal(ref.smooth(hist[:3], np.array([0.2, 0.4, np.nan], np.float32), ref.zero_state(), 0.5, 4000)[3][:256], hist[2])


def test_restatement_batching_does_not_matter():
    """N frames in batches of 1, 3 and N: the same bits out and the same final state"""
    rng = np.random.default_rng(4)
    N = 11
    hist = np.concatenate([_hists(rng, 4), _hists(rng, 3, bins=(120, 256)), _hists(rng, 4, bins=(40, 90))])
    r = rng.uniform(0.05, 0.6, size=N).astype(np.float32)
    r[5] = np.nan
    whole = ref.smooth(hist, r, ref.zero_state(), 0.3, 1200)
    assert list(whole[2]) == [1, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0]
    for step in (1, 3):
        state = ref.zero_state()
        outs, dists, cuts = [], [], []
        for s in range(0, N, step):
            o, d, c, state = ref.smooth(hist[s:s + step], r[s:s + step], state, 0.3, 1200)
            outs.append(o), dists.append(d), cuts.append(c)
        assert np.array_equal(np.concatenate(outs).view(np.uint32), whole[0].view(np.uint32)), step
        assert np.array_equal(np.concatenate(dists), whole[1]) and np.array_equal(np.concatenate(cuts), whole[2]), step
        assert np.array_equal(state, whole[3]), step


def test_scene_frames_cut_where_they_should():
    """the frames of the GPU wiring tests, on the restatement alone: the two scenes are further apart than the default threshold, the two
    frames of one scene are not"""
    for bits in (8, 10):
        frames = ref.scene_frames(bits=bits)
        assert frames.shape == (4, 34 * 38 * 3 // 2)
        hist = ref.luma_hist(frames, 34, 38, bits)
        above = ref.cut_above(0.3, 34, 38)
        assert above == 775
        _, dist, cut, _ = ref.smooth(hist, np.full(4, 0.3, np.float32), ref.zero_state(), 0.25, above)
        print(f"{bits} bit: distances {list(dist)}, threshold {above}")
        assert list(cut) == [1, 0, 1, 0] and dist[2] == 2 * 34 * 38 and dist[1] < above // 2 and dist[3] < above // 2


def test_ratio_filter_checks_its_arguments():
    from fdn_hip import FdnHipError
    from fdn_hip.temporal import RatioFilter
    f = RatioFilter(34, 38, 8, 0.25, device="cpu")                                 # the state is plain memory until step() is called
    assert (f.h, f.w, f.bits, f.alpha, f.cut, f.cut_above) == (34, 38, 8, 0.25, 0.3, 775)
    assert f.state.shape == (258,) and int(f.state.abs().sum()) == 0 and f.cuts_seen() == 0 and f.last_cut is None and f.last_dist is None
    assert RatioFilter(34, 38, 8, 1.0, cut=1.0, device="cpu").cut_above == 2 * 34 * 38
    assert RatioFilter(34, 38, 8, 1.0, cut=0.0, device="cpu").cut_above == 0
    assert RatioFilter(720, 1280, 10, 0.5, cut=0.5, device="cpu").cut_above == 720 * 1280
    for h, w, bits, alpha, cut in ((34, 38, 8, 0.25, 0.3), (720, 1280, 10, 0.1, 0.7), (2, 2, 8, 1.0, 0.99)):
        assert RatioFilter(h, w, bits, alpha, cut=cut, device="cpu").cut_above == ref.cut_above(cut, h, w)
    for kw in (dict(alpha=0.0), dict(alpha=-0.5), dict(alpha=1.5), dict(alpha=float("nan")), dict(cut=-0.1), dict(cut=1.1),
               dict(cut=float("nan")), dict(bits=12), dict(bits=16), dict(h=33), dict(w=37), dict(h=0), dict(h=32768, w=32768)):
        args = dict(h=34, w=38, bits=8, alpha=0.25, cut=0.3)
        args.update(kw)
        with pytest.raises(ValueError):
            RatioFilter(device="cpu", **args)
    # no host fallback: well-formed frames on the CPU are refused, and so are badly formed ones, before any launch
    n = 34 * 38 * 3 // 2
    r = torch.full((2, 1), 0.3)
    with pytest.raises(FdnHipError, match="ROCm"):
        f.step(torch.zeros(2, n, dtype=torch.uint8), r)
    with pytest.raises(FdnHipError, match="frames must be"):
        f.step(torch.zeros(2, n, dtype=torch.int16), r)
    with pytest.raises(FdnHipError, match="expected frames"):
        f.step(torch.zeros(2, n - 1, dtype=torch.uint8), r)


def test_enhance_yuv420_refuses_what_cannot_be_filtered(lib):
    import inspect
    from fdn_hip import harness
    from fdn_hip.temporal import RatioFilter
    assert inspect.signature(harness.enhance_yuv420).parameters["temporal"].default is None
    fmt8, fmt10 = harness.VideoFormat("yuv420p"), harness.VideoFormat("yuv420p10le")
    n = fmt8.frame_samples(34, 38)
    frames = torch.zeros(2, n, dtype=torch.uint8)
    f = RatioFilter(34, 38, 8, 0.25, device="cpu")
    with pytest.raises(ValueError, match="fixed"):
        harness.enhance_yuv420(None, None, frames, 34, 38, fmt8, ratio_mode="fixed", ratio=torch.ones(2, 1), temporal=f)
    for tile in (None, (32, 32)):
        with pytest.raises(ValueError, match="ratio_from"):
            harness.enhance_yuv420(None, None, frames, 34, 38, fmt8, tile=tile, ratio_from="tile", temporal=f)
    with pytest.raises(ValueError, match="10-bit"):
        harness.enhance_yuv420(None, None, torch.zeros(2, n, dtype=torch.int16), 34, 38, fmt10, temporal=f)
    with pytest.raises(ValueError, match="34x38"):
        harness.enhance_yuv420(None, None, torch.zeros(2, 36 * 38 * 3 // 2, dtype=torch.uint8), 36, 38, fmt8, temporal=f)
    with pytest.raises(ValueError, match="34x38"):
        harness.enhance_yuv420(None, None, torch.zeros(2, 34 * 40 * 3 // 2, dtype=torch.uint8), 34, 40, fmt8, temporal=f)


def test_driver_flags():
    import inference_fdn_video as drv
    base = ["--fdn", "F.pth", "--lpnet", "L.pth", "in.y4m", "out.y4m"]
    a = drv.parse_args(base)
    assert a.ratio_smooth is None and a.scene_cut == 0.3                            # off by default
    a = drv.parse_args(base + ["--ratio-smooth", "0.25"])
    assert a.ratio_smooth == 0.25 and a.scene_cut == 0.3
    a = drv.parse_args(base + ["--ratio-smooth", "1", "--scene-cut", "0.5"])
    assert a.ratio_smooth == 1.0 and a.scene_cut == 0.5
    assert drv.parse_args(base + ["--ratio-smooth", "0.5", "--scene-cut", "0"]).scene_cut == 0.0
    assert drv.parse_args(base + ["--ratio-smooth", "0.5", "--scene-cut", "1"]).scene_cut == 1.0
    assert drv.parse_args(base + ["--ratio-smooth", "1e-3"]).ratio_smooth == 1e-3
    for bad in (["--ratio-smooth", "0"], ["--ratio-smooth", "-0.1"], ["--ratio-smooth", "1.5"], ["--ratio-smooth", "x"],
                ["--ratio-smooth", "nan"], ["--ratio-smooth"], ["--scene-cut", "-0.1"], ["--scene-cut", "1.1"], ["--scene-cut", "nan"],
                ["--ratio-smooth", "0.5", "--tile-ratio", "tile"], ["--batch", "0"]):
        with pytest.raises(SystemExit):
            drv.parse_args(base + bad)
    assert drv.parse_args(base + ["--tile-ratio", "tile"]).tile_ratio == "tile"     # without the filter, as before
