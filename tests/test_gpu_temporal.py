"""GPU: the ratio filter across frames - fdn_luma_hist / fdn_ratio_smooth (include/fdn_temporal.h), fdn_hip.temporal.RatioFilter,
fdn_hip.harness.enhance_yuv420(temporal=...) and inference_fdn_video.py --ratio-smooth.

The reference has nothing of the kind, so the yardstick is the restatement of tests/temporal_ref.py.  Everything the two kernels decide is
decided on integers, and the filter is three float32 operations rounded once each, so every comparison here is for equality: histograms,
distances and cut flags as integers, filtered ratios and the carried state bit for bit.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import temporal_ref as ref
from common import fdn_weights, lpnet_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fdn-tip2025_amd")

from common import poison_uninitialized  # noqa: F401  (autouse, tests/common.py: torch.empty is filled with NaN / the integer maximum)
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Hn():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import fdn_hip
    fdn_hip.lib()   # fail loudly if the HIP extension is not built
    from fdn_hip import harness
    return harness


def cuda(a):
    """numpy or torch -> a contiguous tensor on the GPU; unsigned 16- and 32-bit values travel as int16 / int32"""
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(a.view({np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}.get(a.dtype, a.dtype)))
    return a.to("cuda:0").contiguous()


def host(t):
    """a frames tensor -> numpy, 16-bit samples as uint16"""
    a = t.cpu().contiguous()
    return a.view(torch.int16).numpy().view(np.uint16) if a.dtype != torch.uint8 else a.numpy()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def gpu_hist(frames, h, w, bits):
    """fdn_luma_hist on device frames [B, n] into a histogram pre-filled with garbage -> uint32 [B, 256]"""
    import fdn_hip
    B = frames.shape[0]
    hist = torch.full((B, 256), -123456789, dtype=torch.int32, device=frames.device)
    fdn_hip.check(fdn_hip.lib().fdn_luma_hist(ptr(frames), ptr(hist), B, h, w, bits, fdn_hip.stream()), "fdn_luma_hist")
    return hist.cpu().numpy().view(np.uint32)


def check_hist(frames, h, w, bits, dev=None):
    want = ref.luma_hist(frames, h, w, bits)
    got = gpu_hist(cuda(frames) if dev is None else dev, h, w, bits)
    assert np.all(want.sum(axis=1) == h * w) and np.all(got.sum(axis=1, dtype=np.int64) == h * w)
    assert np.array_equal(got, want)
    return got


def codes(rng, B, h, w, bits, lo=0, hi=None):
    hi = 2 ** bits if hi is None else hi
    return rng.integers(lo, hi, size=(B, h * w * 3 // 2)).astype(np.uint8 if bits == 8 else np.uint16)


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("shape", [(2, 2, 1), (6, 10, 3), (34, 514, 2)], ids=["2x2", "6x10x3", "34x514x2"])
def test_hist_shapes(Hn, shape, bits):
    """2 x 2: four samples, only the sample-by-sample path.  6 x 10, B = 3: frames start at samples 90 and 180, off every 4- and 16-byte
    boundary, so the path before the first whole vector runs and a frame's samples must not leak into its neighbour's row.  34 x 514,
    B = 2: a plane of 17,476 samples - whole vectors, a remainder, several workgroups per frame, the batch stride."""
    h, w, B = shape
    rng = np.random.default_rng(10 * h + bits)
    frames = codes(rng, B, h, w, bits)
    got = check_hist(frames, h, w, bits)
    if B > 1:
        assert not np.array_equal(got[0], got[1])
    # dark footage: nearly all samples in a handful of bins
    check_hist(codes(rng, B, h, w, bits, lo=16 * 2 ** (bits - 8), hi=20 * 2 ** (bits - 8)), h, w, bits)


@pytest.mark.parametrize("bits", [8, 10])
def test_hist_unaligned_base(Hn, bits):
    """frames that start one sample after an allocation's base: frame 0 too begins off the 16-byte grid"""
    rng = np.random.default_rng(20 + bits)
    h, w, B = 6, 38, 2
    frames = codes(rng, B, h, w, bits)
    n = frames.shape[1]
    flat = cuda(np.concatenate([frames[0, :1], frames.reshape(-1)]))
    dev = flat[1:].view(B, n)
    assert dev.is_contiguous() and dev.data_ptr() % 16 == frames.itemsize
    check_hist(frames, h, w, bits, dev=dev)


@pytest.mark.parametrize("bits", [8, 10])
def test_hist_one_and_two_bins(Hn, bits):
    """64 x 96 with every luma sample at code 17 (x 4 at 10 bit), then a checkerboard of two codes: every increment of a wave lands on one
    or two words, so an update lost between lanes or waves would show"""
    h, w, s = 64, 96, 2 ** (bits - 8)
    dt = np.uint8 if bits == 8 else np.uint16
    chroma = np.full(h * w // 2, 128 * s)
    flat = np.concatenate([np.full(h * w, 17 * s), chroma]).astype(dt)[None]
    got = check_hist(flat, h, w, bits)
    assert got[0, 17] == h * w and np.count_nonzero(got) == 1
    yy, xx = np.mgrid[:h, :w]
    board = np.where((yy + xx) % 2 == 0, 17 * s, 203 * s).reshape(-1)
    got = check_hist(np.concatenate([board, chroma]).astype(dt)[None], h, w, bits)
    assert got[0, 17] == got[0, 203] == h * w // 2 and np.count_nonzero(got) == 2


def test_hist_ten_bit_words_above_1023(Hn):
    """1023, 1024 and 65535 all land in bin 255"""
    h, w = 6, 10
    frames = np.zeros((1, h * w * 3 // 2), dtype=np.uint16)
    frames[0, :h * w] = np.resize(np.array([1023, 1024, 65535, 1020, 1019, 4, 3], dtype=np.uint16), h * w)
    got = check_hist(frames, h, w, 10)
    per = {v: int((frames[0, :h * w] == v).sum()) for v in (1023, 1024, 65535, 1020, 1019, 4, 3)}
    assert got[0, 255] == per[1023] + per[1024] + per[65535] + per[1020] and got[0, 254] == per[1019]
    assert got[0, 1] == per[4] and got[0, 0] == per[3]


def test_hist_never_counts_chroma(Hn):
    """planar and nv12 frames share the luma plane; chroma samples all at code 200, a code absent from luma, leave bin 200 empty"""
    import yuv_ref
    h, w, B = 18, 22, 2
    rng = np.random.default_rng(33)
    y = rng.integers(0, 200, size=(B, h, w))
    c = np.full((B, h // 2, w // 2), 200)
    planar, nv12 = yuv_ref.pack(y, c, c, "yuv420p"), yuv_ref.pack(y, c, c, "nv12")
    a, b = check_hist(planar, h, w, 8), check_hist(nv12, h, w, 8)
    assert np.array_equal(a, b) and np.all(a[:, 200] == 0)
    y10 = rng.integers(0, 800, size=(B, h, w))
    ten = yuv_ref.pack(y10, np.full_like(c, 803), np.full_like(c, 803), "yuv420p10le")
    assert np.all(check_hist(ten, h, w, 10)[:, 200] == 0)


# --------------------------------------------------------------------------------------------------------------------------------
# fdn_ratio_smooth on histograms crafted as integers
# --------------------------------------------------------------------------------------------------------------------------------
def gpu_smooth(hist, ratio, state, alpha, cut_above):
    """-> (ratio_out float32 [B], dist uint32 [B], cut int32 [B], state uint32 [258]) from the kernel; outputs pre-filled with garbage"""
    import fdn_hip
    B = hist.shape[0]
    d_hist, d_ratio, d_state = cuda(np.ascontiguousarray(hist, dtype=np.uint32)), cuda(np.asarray(ratio, dtype=np.float32)), cuda(state.copy())
    out = torch.full((B,), -7.0, dtype=torch.float32, device="cuda:0")
    dist = torch.full((B,), -5, dtype=torch.int32, device="cuda:0")
    cut = torch.full((B,), -5, dtype=torch.int32, device="cuda:0")
    fdn_hip.check(fdn_hip.lib().fdn_ratio_smooth(ptr(d_hist), ptr(d_ratio), ptr(d_state), alpha, cut_above, B, ptr(out), ptr(dist), ptr(cut),
                                                 fdn_hip.stream()), "fdn_ratio_smooth")
    return out.cpu().numpy(), dist.cpu().numpy().view(np.uint32), cut.cpu().numpy(), d_state.cpu().numpy().view(np.uint32)


def same(got, want):
    """(ratio_out, dist, cut, state) of the kernel against the restatement's: integers equal, floats bit for bit"""
    assert np.array_equal(got[1], want[1]), (got[1], want[1])
    assert np.array_equal(got[2], want[2]), (got[2], want[2])
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), (got[0], want[0])
    assert np.array_equal(got[3], want[3])


def hists(rng, B, total=2000, bins=(0, 100)):
    return np.stack([np.bincount(rng.integers(bins[0], bins[1], size=total), minlength=256) for _ in range(B)]).astype(np.uint32)


def ratios(rng, B):
    return rng.uniform(0.05, 0.6, size=B).astype(np.float32)


def test_smooth_first_frame(Hn):
    rng = np.random.default_rng(40)
    hist, r = hists(rng, 1), ratios(rng, 1)
    want = ref.smooth(hist, r, ref.zero_state(), 0.25, 1200)
    assert list(want[2]) == [1] and want[1][0] == 0 and want[0][0] == r[0] and want[3][257] == 3
    same(gpu_smooth(hist, r, ref.zero_state(), 0.25, 1200), want)


@pytest.mark.parametrize("alpha", [0.25, 1.0, 2.0 ** -6])
def test_smooth_five_frames_with_a_cut(Hn, alpha):
    """histograms disjoint from frame 3 on; also alpha = 1 (nothing filtered, cuts still found) and a small alpha"""
    rng = np.random.default_rng(41)
    hist = np.concatenate([hists(rng, 3), hists(rng, 2, bins=(150, 250))])
    r = ratios(rng, 5)
    want = ref.smooth(hist, r, ref.zero_state(), alpha, 1200)
    assert list(want[2]) == [1, 0, 0, 1, 0] and want[1][3] == 4000
    if alpha == 1.0:
        assert np.array_equal(want[0], r)
    else:
        assert want[0][1] != r[1] and want[0][3] == r[3]
    same(gpu_smooth(hist, r, ref.zero_state(), alpha, 1200), want)


def test_smooth_threshold_edge(Hn):
    """dist == cut_above is no cut, dist == cut_above + 1 is one"""
    rng = np.random.default_rng(42)
    hist, r = hists(rng, 2), ratios(rng, 2)
    d = int(np.abs(hist[1].astype(np.int64) - hist[0].astype(np.int64)).sum())
    assert d > 1
    for above, flag in ((d, 0), (d - 1, 1), (0, 1), (2 ** 31 - 1, 0)):
        want = ref.smooth(hist, r, ref.zero_state(), 0.5, above)
        assert want[1][1] == d and want[2][1] == flag
        same(gpu_smooth(hist, r, ref.zero_state(), 0.5, above), want)
    # identical frames: distance 0 is no cut even at cut_above = 0
    twice = np.stack([hist[0], hist[0]])
    want = ref.smooth(twice, r, ref.zero_state(), 0.5, 0)
    assert list(want[1]) == [0, 0] and list(want[2]) == [1, 0]
    same(gpu_smooth(twice, r, ref.zero_state(), 0.5, 0), want)


@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_smooth_non_finite_in_the_middle(Hn, bad):
    rng = np.random.default_rng(43)
    hist, r = hists(rng, 5), ratios(rng, 5)
    r[2] = bad
    want = ref.smooth(hist, r, ref.zero_state(), 0.5, 4000)
    assert not np.isfinite(want[0][2]) and np.all(np.isfinite(want[0][[0, 1, 3, 4]])) and want[0][3] != r[3]
    same(gpu_smooth(hist, r, ref.zero_state(), 0.5, 4000), want)
    first = r.copy()
    first[:2] = np.nan                                                              # no ratio in the state until frame 3
    want = ref.smooth(hist, first, ref.zero_state(), 0.5, 4000)
    assert want[0][3] == first[3]
    same(gpu_smooth(hist, first, ref.zero_state(), 0.5, 4000), want)


def test_smooth_state_carries_across_calls(Hn):
    """3 + 2 frames in two calls = 5 in one call, with the cut on either side of the seam"""
    rng = np.random.default_rng(44)
    for split in (3, 2):
        hist = np.concatenate([hists(rng, 3), hists(rng, 2, bins=(150, 250))])
        r = ratios(rng, 5)
        whole = ref.smooth(hist, r, ref.zero_state(), 0.25, 1200)
        a = gpu_smooth(hist[:split], r[:split], ref.zero_state(), 0.25, 1200)
        same(a, ref.smooth(hist[:split], r[:split], ref.zero_state(), 0.25, 1200))
        b = gpu_smooth(hist[split:], r[split:], a[3], 0.25, 1200)
        same(tuple(np.concatenate([x, y]) for x, y in zip(a[:3], b[:3])) + (b[3],), whole)
        same(gpu_smooth(hist, r, ref.zero_state(), 0.25, 1200), whole)


def test_smooth_more_frames_than_threads(Hn):
    """B = 300: scenes of random length, a NaN here and there"""
    rng = np.random.default_rng(45)
    parts, left = [], 300
    while left:
        k = min(left, int(rng.integers(1, 40)))
        lo = int(rng.integers(0, 150))
        parts.append(hists(rng, k, bins=(lo, lo + 100)))
        left -= k
    hist = np.concatenate(parts)
    r = ratios(rng, 300)
    r[[17, 18, 120, 299]] = np.nan
    want = ref.smooth(hist, r, ref.zero_state(), 0.125, 1200)
    assert 5 < want[2].sum() < 150
    same(gpu_smooth(hist, r, ref.zero_state(), 0.125, 1200), want)


# --------------------------------------------------------------------------------------------------------------------------------
# wiring: RatioFilter, enhance_yuv420(temporal=...), the driver
# --------------------------------------------------------------------------------------------------------------------------------
def load(mod, sd):
    mod.load_state_dict(sd, strict=True)
    return mod.to("cuda:0").eval()


@pytest.fixture(scope="module")
def nets(Hn):
    from basicsr.models.archs.FDN_arch import FDN
    from basicsr.models.archs.LPNet_arch import I_predict_net
    return load(FDN(), fdn_weights(tame=0.03)), load(I_predict_net(), lpnet_weights())


def expected_flags(frames, h, w, bits, cut=0.3):
    """the restatement's cut flags and distances of host frames from the reset state; checked before the kernel is judged"""
    _, dist, flags, _ = ref.smooth(ref.luma_hist(frames, h, w, bits), np.full(frames.shape[0], 0.3, np.float32), ref.zero_state(), 0.25,
                                   ref.cut_above(cut, h, w))
    return flags, dist


@pytest.mark.parametrize("bits", [8, 10])
def test_ratio_filter_steps(Hn, bits):
    """RatioFilter on the four scene frames, whole and frame by frame: the restatement's ratios, flags, distances and state"""
    from fdn_hip.temporal import RatioFilter
    frames = ref.scene_frames(bits=bits)
    flags, dist = expected_flags(frames, 34, 38, bits)
    assert list(flags) == [1, 0, 1, 0] and dist[2] > 775 > dist[1] and dist[3] < 775
    r = np.array([0.31, 0.27, 0.52, 0.47], dtype=np.float32)
    want = ref.smooth(ref.luma_hist(frames, 34, 38, bits), r, ref.zero_state(), 0.25, 775)
    f = RatioFilter(34, 38, bits, 0.25, device="cuda:0")
    assert f.cut_above == 775 and f.cuts_seen() == 0
    dev = cuda(frames)
    got = f.step(dev, cuda(r).reshape(4, 1))
    assert got.shape == (4, 1) and got.dtype == torch.float32
    same((got.cpu().numpy().reshape(-1), f.last_dist.cpu().numpy().view(np.uint32), f.last_cut.cpu().numpy(),
          f.state.cpu().numpy().view(np.uint32)), want)
    assert f.cuts_seen() == 2
    f.reset()
    assert f.cuts_seen() == 0 and int(f.state.abs().sum()) == 0
    one = torch.cat([f.step(dev[t] if bits == 8 else dev[t].view(torch.uint16), cuda(r[t:t + 1]).reshape(1, 1)) for t in range(4)])
    assert torch.equal(one, got) and f.cuts_seen() == 2 and np.array_equal(f.state.cpu().numpy().view(np.uint32), want[3])
    with pytest.raises(Hn.FdnHipError, match="ratio must be"):
        f.step(dev, cuda(r))


@pytest.mark.parametrize("mode", ["lolblur", "lolv1"])
def test_enhance_untiled_with_filter(Hn, nets, mode):
    """enhance_yuv420(temporal=f) = enhance_yuv420(ratio_mode="fixed", ratio=the filter's output for that batch), sample for sample: the same
    launches on the same ratio bits.  The filter is fed what FDN would have been fed, and it changes the frames that follow a frame of
    their scene."""
    from fdn_hip.temporal import RatioFilter
    net, lp = nets
    fmt = Hn.VideoFormat("yuv420p", "bt601", False, "left")
    host_frames = ref.scene_frames()
    flags, _ = expected_flags(host_frames, 34, 38, 8)
    assert list(flags) == [1, 0, 1, 0]
    frames = cuda(host_frames)
    f = RatioFilter(34, 38, 8, 0.25, device="cuda:0")
    got = Hn.enhance_yuv420(net, lp, frames, 34, 38, fmt, ratio_mode=mode, temporal=f)
    assert got.shape == frames.shape and got.dtype == torch.uint8
    assert np.array_equal(f.last_cut.cpu().numpy(), flags) and f.cuts_seen() == 2
    with torch.no_grad():
        raw = Hn.frame_ratio(lp, Hn.preprocess_yuv420(frames, 34, 38, fmt)[0], mode).contiguous()
    f_out = RatioFilter(34, 38, 8, 0.25, device="cuda:0").step(frames, raw)
    want_r = ref.smooth(ref.luma_hist(host_frames, 34, 38, 8), raw.cpu().numpy().reshape(-1), ref.zero_state(), 0.25, 775)[0]
    assert np.array_equal(f_out.cpu().numpy().reshape(-1).view(np.uint32), want_r.view(np.uint32))
    assert f_out[0, 0] == raw[0, 0] and f_out[2, 0] == raw[2, 0]                   # cuts: the frame's own ratio
    print(f"{mode}: raw {raw.reshape(-1).tolist()} filtered {f_out.reshape(-1).tolist()}")
    fixed = Hn.enhance_yuv420(net, None, frames, 34, 38, fmt, ratio_mode="fixed", ratio=f_out)
    assert torch.equal(got, fixed)
    # a second batch continues the stream: no cut at its first frame, which is filtered against the state
    again = Hn.enhance_yuv420(net, lp, frames[3:], 34, 38, fmt, ratio_mode=mode, temporal=f)
    assert list(f.last_cut.cpu().numpy()) == [0] and f.cuts_seen() == 2 and again.shape == (1, frames.shape[1])


def test_enhance_tiled_with_filter(Hn, nets):
    """two 70 x 90 frames of one scene, tile (32, 64), ratio_from "frame": the frame's filtered ratio goes to every tile"""
    from fdn_hip.temporal import RatioFilter
    net, lp = nets
    h, w = 70, 90
    fmt = Hn.VideoFormat("yuv420p", "bt709", False, "left")
    host_frames = ref.scene_frames(seed=9, h=h, w=w)[:2]
    flags, _ = expected_flags(host_frames, h, w, 8)
    assert list(flags) == [1, 0]
    frames = cuda(host_frames)
    f = RatioFilter(h, w, 8, 0.25, device="cuda:0")
    got = Hn.enhance_yuv420(net, lp, frames, h, w, fmt, tile=(32, 64), ratio_from="frame", batch=4, temporal=f)
    assert got.shape == frames.shape and f.cuts_seen() == 1 and list(f.last_cut.cpu().numpy()) == [0]
    with torch.no_grad():
        raw = torch.cat([Hn.frame_ratio(lp, Hn.preprocess_yuv420(frames[b:b + 1], h, w, fmt)[0], "lolblur") for b in range(2)]).contiguous()
    f_out = RatioFilter(h, w, 8, 0.25, device="cuda:0").step(frames, raw)
    assert f_out[0, 0] == raw[0, 0]
    fixed = Hn.enhance_yuv420(net, None, frames, h, w, fmt, ratio_mode="fixed", ratio=f_out, tile=(32, 64), ratio_from="frame", batch=4)
    assert torch.equal(got, fixed)


def test_driver_ratio_smooth(Hn, nets, tmp_path):
    """the four scene frames as Y4M through pipes with --ratio-smooth 0.25: the harness's bytes, and `2 scene cuts` on stderr"""
    from fdn_hip.temporal import RatioFilter
    net, lp = nets
    torch.save({"params": fdn_weights(tame=0.03)}, tmp_path / "fdn.pth")
    torch.save({"params": lpnet_weights()}, tmp_path / "lpnet.pth")
    frames = ref.scene_frames()
    header = b"YUV4MPEG2 W38 H34 F25:1 Ip A1:1 C420mpeg2\n"
    stream = header + b"".join(b"FRAME\n" + f.tobytes() for f in frames)
    run = subprocess.run([sys.executable, os.path.join(PKG, "inference_fdn_video.py"), "--fdn", str(tmp_path / "fdn.pth"), "--lpnet",
                          str(tmp_path / "lpnet.pth"), "--ratio-smooth", "0.25", "-", "-"], input=stream, capture_output=True, timeout=600)
    err = run.stderr.decode()
    print(err)
    assert run.returncode == 0, err
    assert err.rstrip("\n").split("\n")[-1] == "4 frames -> -, 2 scene cuts"
    fmt = Hn.VideoFormat("yuv420p", "bt601", False, "left")
    f = RatioFilter(34, 38, 8, 0.25, device="cuda:0")
    want = host(Hn.enhance_yuv420(net, lp, cuda(frames), 34, 38, fmt, temporal=f))
    assert run.stdout == header + b"".join(b"FRAME\n" + fr.tobytes() for fr in want)
