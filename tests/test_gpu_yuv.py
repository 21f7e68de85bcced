"""GPU: video frames in and out - fdn_pre_yuv420 / fdn_post_yuv420 (include/fdn_video.h), fdn_hip.harness.preprocess_yuv420 /
postprocess_yuv420 / enhance_yuv420 and the inference_fdn_video.py driver.

The reference has nothing of the kind, so the yardstick is the float64 restatement of tests/yuv_ref.py.  Shapes h x w -> H x W
(yuv_ref.SHAPES), each over {yuv420p, nv12, yuv420p10le} x {bt601, bt709} x {limited, full} x {left, center}:

    2 x 2    -> 2 x 2            one chroma sample: every interpolation and filter tap is clamped
    2 x 4    -> 2 x 4            two chroma columns, still clamped at both ends
    18 x 22  -> 32 x 32          reflection on both axes
    34 x 38  -> 64 x 64          pads of 30 and 26, close to the pad < size limit: the reflection reaches far back
    34 x 514 -> 64 x 544, B = 2  three blocks of 256 per row with a partial last one, and the batch stride

Bounds.  pre: |got - ref| <= 2e-6.  A value passes through at most about twelve fp32 roundings (subtract and divide per sample, up to four
interpolation taps, the matrix products, three constants rounded to fp32), each at most 2^-24 relative on magnitudes no larger than about
2.3 before the clamp: about 1.6e-6.  post: every sample equals the restatement's code, except that where the float64 value before rounding
lies within 1e-3 code units of a half one code of difference is allowed: about twelve roundings on values up to 1023, ulp 6.1e-5, is about
7.3e-4.  Under 1 % of a case's samples may lie in that window, which is checked on the restatement alone before the kernel is judged.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import yuv_ref as ref
from common import fdn_weights, lpnet_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fdn-tip2025_amd")

from common import poison_uninitialized  # noqa: F401  (autouse, tests/common.py: torch.empty is filled with NaN / the integer maximum)
pytestmark = pytest.mark.gpu

IDS = [f"{h}x{w}" for h, w, _, _, _ in ref.SHAPES]
PRE_BOUND = 2e-6


@pytest.fixture(scope="module")
def Hn():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import fdn_hip
    fdn_hip.lib()   # fail loudly if the HIP extension is not built
    from fdn_hip import harness
    return harness


def load(mod, sd):
    mod.load_state_dict(sd, strict=True)
    return mod.to("cuda:0").eval()


@pytest.fixture(scope="module")
def nets(Hn):
    from basicsr.models.archs.FDN_arch import FDN
    from basicsr.models.archs.LPNet_arch import I_predict_net
    return load(FDN(), fdn_weights(tame=0.03)), load(I_predict_net(), lpnet_weights())


def cuda(a):
    """numpy or torch -> a contiguous tensor on the GPU; uint16 samples travel as int16"""
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)
    return a.to("cuda:0").contiguous()


def host(t):
    """a frames tensor -> numpy, 16-bit samples as uint16"""
    a = t.cpu().contiguous()
    return a.view(torch.int16).numpy().view(np.uint16) if a.dtype != torch.uint8 else a.numpy()


def vfmt(Hn, case):
    pix, m, full, loc = case
    return Hn.VideoFormat(pix, m, full, loc)


def name(case):
    pix, m, full, loc = case
    return f"{pix} {m} {'full' if full else 'limited'} {loc}"


def pre_into(Hn, frames, h, w, H, W, case):
    """fdn_pre_yuv420 with the padded size given (the harness pads to the x32 grid only)"""
    import fdn_hip
    pix, m, full, loc = case
    layout, bits = ref.PIX_FMTS[pix]
    out = torch.full((frames.shape[0], 3, H, W), float("nan"), device=frames.device, dtype=torch.float32)
    fdn_hip.check(fdn_hip.lib().fdn_pre_yuv420(ctypes.c_void_p(frames.data_ptr()), ctypes.c_void_p(out.data_ptr()), frames.shape[0], h, w, H, W,
                                               layout, bits, list(ref.MATRICES).index(m), int(full), ["left", "center"].index(loc),
                                               fdn_hip.stream()), "fdn_pre_yuv420")
    return out


@pytest.mark.parametrize("shape", ref.SHAPES, ids=IDS)
def test_pre_against_float64(Hn, shape):
    h, w, H, W, B = shape
    worst = 0.0
    for n, case in enumerate(ref.FORMATS):
        frames = ref.random_frames(100 + n, B, h, w, case[0])                               # codes over the whole code range
        want = ref.pre64(frames, h, w, H, W, *case)
        dev = cuda(frames)
        got = pre_into(Hn, dev, h, w, H, W, case)
        assert got.shape == (B, 3, H, W)
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
        worst = max(worst, err)
        assert err <= PRE_BOUND, (name(case), err)
        assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
        fmt = vfmt(Hn, case)
        plain, hh, ww = Hn.preprocess_yuv420(dev, h, w, fmt, pad=False)
        assert (hh, ww) == (h, w) and plain.shape == (B, 3, h, w) and torch.equal(plain, got[:, :, :h, :w]), name(case)
        if Hn.padded_size(h, w) == (H, W):
            assert torch.equal(Hn.preprocess_yuv420(dev, h, w, fmt)[0], got), name(case)
    print(f"{h}x{w} -> {H}x{W}: largest |got - float64| over {len(ref.FORMATS)} formats {worst:.3e} (bound {PRE_BOUND:.0e})")
    if h == 2:
        with pytest.raises(Hn.FdnHipError, match="pad < size"):
            Hn.preprocess_yuv420(dev, h, w, fmt)                                            # 2 x 2 -> 32 x 32 cannot be reflected


def test_pre_takes_uint16_and_a_single_frame(Hn):
    fmt = Hn.VideoFormat("yuv420p10le")
    frames = ref.random_frames(7, 2, 18, 22, "yuv420p10le")
    as_i16 = cuda(frames)
    want = Hn.preprocess_yuv420(as_i16, 18, 22, fmt)[0]
    assert torch.equal(Hn.preprocess_yuv420(as_i16.view(torch.uint16), 18, 22, fmt)[0], want)
    assert torch.equal(Hn.preprocess_yuv420(as_i16[1], 18, 22, fmt)[0], want[1:])
    with pytest.raises(Hn.FdnHipError, match="contiguous"):
        Hn.preprocess_yuv420(cuda(np.concatenate([frames, frames], axis=1))[:, :frames.shape[1]], 18, 22, fmt)


def test_gamut(Hn):
    """legal and illegal extremes give finite values within [0,1]: out of gamut is clamped, a 10-bit word above 1023 counts as 1023"""
    for h, w, H, W in ((2, 2, 2, 2), (18, 22, 32, 32)):
        n = h * w
        for case in ref.FORMATS:
            pix = case[0]
            s = 2 ** (ref.PIX_FMTS[pix][1] - 8)
            top = 256 * s - 1
            triples = [(235 * s, 240 * s), (16 * s, 16 * s), (0, 0), (top, top), (0, top), (top, 0)] + ([(0xFFFF, 0xFFFF)] if s > 1 else [])
            for yv, cv in triples:
                frames = np.concatenate([np.full((1, n), yv), np.full((1, n // 2), cv)], axis=1).astype(ref.sample_dtype(pix))
                got = pre_into(Hn, cuda(frames), h, w, H, W, case)
                assert bool(torch.isfinite(got).all()) and float(got.min()) >= 0.0 and float(got.max()) <= 1.0, (name(case), yv, cv)
                want = ref.pre64(frames, h, w, H, W, *case)
                assert np.abs(got.cpu().numpy() - want).max() <= PRE_BOUND, (name(case), yv, cv)
                if yv == 0xFFFF:
                    assert torch.equal(got, pre_into(Hn, cuda(np.minimum(frames, 1023)), h, w, H, W, case))
    # the reason for the clamp: Y 235 with Cb = Cr = 240 is a legal triple far outside the gamut
    want = ref.pre64(np.array([[235] * 4 + [240] * 2], dtype=np.uint8), 2, 2, 2, 2, "yuv420p", "bt709", False, "left")
    assert want.max() == 1.0 and want[0, 1].max() < 1.0


@pytest.mark.parametrize("shape", ref.SHAPES, ids=IDS)
def test_post_against_float64(Hn, shape):
    h, w, H, W, B = shape
    res = ref.random_planes(ref.POST_SEED, B, H, W)                                         # fp32 uniform in [-0.2, 1.2]
    assert res.size < 3000 or (res.min() < -0.15 and res.max() > 1.15)
    dev = cuda(res)
    total = 0
    for case in ref.FORMATS:
        want, exact = ref.post64(res, h, w, *case)
        tie = ref.near_tie(exact)
        share = float(tie.mean())
        assert share < 0.01, "the seeded inputs put too many samples next to a tie for the comparison to mean anything"
        fmt = vfmt(Hn, case)
        got_t = Hn.postprocess_yuv420(dev, h, w, fmt)
        assert got_t.shape == (B, h * w * 3 // 2) and got_t.dtype == fmt.dtype
        got = host(got_t)
        off = got != want
        total += int(off.sum())
        print(f"{h}x{w} {name(case)}: {int(tie.sum())} of {tie.size} samples within 1e-3 of a tie ({100 * share:.3f} %), {int(off.sum())} differ")
        assert not np.any(off & ~tie), name(case)
        assert np.all(np.abs(got.astype(np.int64) - want.astype(np.int64)) <= 1), name(case)
    print(f"{h}x{w}: {total} samples differ from the rounded float64 value over {len(ref.FORMATS)} formats")


def test_post_never_reads_the_padding(Hn):
    res = ref.random_planes(11, 2, 64, 64)
    spoiled = res.copy()
    spoiled[:, :, 34:] = np.nan
    spoiled[:, :, :, 38:] = np.inf
    for case in ref.FORMATS:
        fmt = vfmt(Hn, case)
        assert torch.equal(Hn.postprocess_yuv420(cuda(spoiled), 34, 38, fmt), Hn.postprocess_yuv420(cuda(res), 34, 38, fmt)), name(case)


def _round_trip(Hn, frames, h, w, H, W, case):
    dev = cuda(frames)
    back = Hn.postprocess_yuv420(pre_into(Hn, dev, h, w, H, W, case), h, w, vfmt(Hn, case))
    return host(back)


def test_grey_codes_round_trip_exactly(Hn):
    """post(pre(frames)) == frames over all legal grey codes with neutral chroma, 8 and 10 bit, every format"""
    for case in ref.FORMATS:
        pix, _, full, _ = case
        bits = ref.PIX_FMTS[pix][1]
        s = 2 ** (bits - 8)
        codes = np.arange(0, 2 ** bits) if full else np.arange(16 * s, 235 * s + 1)
        w = 2 * ((len(codes) + 1) // 2)
        c = np.full((1, 1, w // 2), 128 * s)
        frames = ref.pack(np.resize(codes, (1, 2, w)), c, c, pix)
        assert set(np.unique(frames[0, :2 * w])) == set(codes)
        x = pre_into(Hn, cuda(frames), 2, w, 2, w, case)
        assert torch.equal(x[:, 0], x[:, 1]) and torch.equal(x[:, 1], x[:, 2])             # neutral chroma: R = G = B
        assert np.array_equal(_round_trip(Hn, frames, 2, w, 2, w, case), frames), name(case)


@pytest.mark.parametrize("shape", ref.SHAPES, ids=IDS)
def test_in_gamut_frames_round_trip_exactly(Hn, shape):
    """random luma in 64 .. 192 (x s) with frame-constant chroma within +-8 (x s) of neutral stays in gamut, so no clamp interferes"""
    h, w, H, W, B = shape
    for n, case in enumerate(ref.FORMATS):
        pix = case[0]
        s = 2 ** (ref.PIX_FMTS[pix][1] - 8)
        rng = np.random.default_rng(300 + n)
        y = rng.integers(64 * s, 192 * s + 1, size=(B, h, w))
        u = np.broadcast_to(128 * s + rng.integers(-8 * s, 8 * s + 1, size=(B, 1, 1)), (B, h // 2, w // 2))
        v = np.broadcast_to(128 * s + rng.integers(-8 * s, 8 * s + 1, size=(B, 1, 1)), (B, h // 2, w // 2))
        frames = ref.pack(y, u, v, pix)
        x = ref.pre64(frames, h, w, h, w, *case)
        assert 0.0 < x.min() and x.max() < 1.0
        assert np.array_equal(_round_trip(Hn, frames, h, w, H, W, case), frames), name(case)


def video_frames(seed, B, h, w, pix):
    """dim, textured frames: luma in the lower half of the range, chroma near neutral"""
    s = 2 ** (ref.PIX_FMTS[pix][1] - 8)
    rng = np.random.default_rng(seed)
    y = rng.integers(20 * s, 110 * s, size=(B, h * w))
    c = rng.integers(112 * s, 144 * s, size=(B, h * w // 2))
    return np.concatenate([y, c], axis=1).astype(ref.sample_dtype(pix))


@pytest.mark.parametrize("pix", ["yuv420p", "yuv420p10le"])
def test_enhance_untiled(Hn, nets, pix):
    """enhance_yuv420 on a 34 x 38 batch of two = postprocess_yuv420(net(preprocess_yuv420(.))) with LPNet's ratio, bit for bit"""
    net, lp = nets
    fmt = Hn.VideoFormat(pix, "bt601", False, "left")
    frames = cuda(video_frames(41, 2, 34, 38, pix))
    got = Hn.enhance_yuv420(net, lp, frames, 34, 38, fmt)
    assert got.shape == frames.shape and got.dtype == frames.dtype
    with torch.no_grad():
        x, h, w = Hn.preprocess_yuv420(frames, 34, 38, fmt)
        assert x.shape == (2, 3, 64, 64)
        ratio = lp(x)
        res = net(x, ratio_i=ratio, device=x.device)[0].contiguous()
    assert bool(torch.isfinite(res).all())
    assert torch.equal(got, Hn.postprocess_yuv420(res, h, w, fmt))
    assert not torch.equal(got, frames)
    # the other ratio modes take the same road
    fixed = Hn.enhance_yuv420(net, None, frames, 34, 38, fmt, ratio_mode="fixed", ratio=ratio)
    assert torch.equal(fixed, got)
    with torch.no_grad():
        res1 = net(x, ratio_i=Hn.lolv1_ratio(x, lp(x)), device=x.device)[0].contiguous()
    assert torch.equal(Hn.enhance_yuv420(net, lp, frames, 34, 38, fmt, ratio_mode="lolv1"), Hn.postprocess_yuv420(res1, h, w, fmt))
    if pix == "yuv420p10le":
        as_u16 = Hn.enhance_yuv420(net, lp, frames.view(torch.uint16), 34, 38, fmt)
        assert as_u16.dtype == torch.uint16 and torch.equal(as_u16.view(torch.int16), got)


@pytest.mark.parametrize("blend", ["average", "feather"])
def test_enhance_tiled(Hn, nets, blend):
    """a 64 x 96 frame with tile (32, 64), overlap 16 = preprocess_yuv420(pad=False) -> split -> run_tiles -> merge -> postprocess_yuv420"""
    from fdn_hip import tiling
    net, lp = nets
    h, w = 64, 96
    fmt = Hn.VideoFormat("yuv420p", "bt709", False, "left")
    frames = cuda(video_frames(51, 2, h, w, "yuv420p"))
    for ratio_from in ("frame", "tile"):
        got = Hn.enhance_yuv420(net, lp, frames, h, w, fmt, tile=(32, 64), overlap=16, blend=blend, ratio_from=ratio_from, batch=4)
        assert got.shape == frames.shape and got.dtype == torch.uint8
        for b in range(2):
            with torch.no_grad():
                x = Hn.preprocess_yuv420(frames[b:b + 1], h, w, fmt, pad=False)[0]
                tiles, ij = tiling.split(x, 32, 64, 16)
                assert tiles.shape[0] == len(tiling.tile_origins(h, w, 32, 64, 16)) == 6   # rows 0, 16, 32; columns 0, 32
                if ratio_from == "frame":
                    r = lp(Hn.preprocess_yuv420(frames[b:b + 1], h, w, fmt)[0]).expand(6, 1).contiguous()
                else:
                    r = torch.cat([lp(tiles[:4]), lp(tiles[4:])])                            # as the forward takes them: batch 4
                outs = tiling.run_tiles(net, tiles, r, 4)
                merged = tiling.merge(outs, ij, h, w, blend=blend)
            assert bool(torch.isfinite(merged).all())
            assert torch.equal(got[b:b + 1], Hn.postprocess_yuv420(merged, h, w, fmt)), (ratio_from, b)


def test_enhance_u8_has_not_moved(Hn, nets):
    """enhance_u8 on an RGB frame gives what preprocess -> LPNet -> FDN -> postprocess gives, as before its forward was shared"""
    net, lp = nets
    img = cuda((torch.rand(2, 34, 38, 3, generator=torch.Generator().manual_seed(61)) * 120).to(torch.uint8))
    with torch.no_grad():
        x, h, w = Hn.preprocess(img, bgr=False)
        res = net(x, ratio_i=lp(x), device=x.device)[0].contiguous()
        res1 = net(x, ratio_i=Hn.lolv1_ratio(x, lp(x)), device=x.device)[0].contiguous()
    assert torch.equal(Hn.enhance_u8(net, lp, img, bgr=False), Hn.postprocess(res, h, w, bgr=False))
    assert torch.equal(Hn.enhance_u8(net, lp, img, bgr=False, ratio_mode="lolv1"), Hn.postprocess(res1, h, w, bgr=False))


@pytest.fixture(scope="module")
def checkpoints(tmp_path_factory):
    d = tmp_path_factory.mktemp("video")
    torch.save({"params": fdn_weights(tame=0.03)}, d / "fdn.pth")
    torch.save({"params": lpnet_weights()}, d / "lpnet.pth")
    return d


def _drive(d, *args, stdin=None):
    return subprocess.run([sys.executable, os.path.join(PKG, "inference_fdn_video.py"), "--fdn", str(d / "fdn.pth"), "--lpnet", str(d / "lpnet.pth"),
                           *args], input=stdin, capture_output=True, timeout=600)


def test_driver_raw_file_to_file(Hn, nets, checkpoints):
    """three 34 x 38 nv12 frames, raw, --batch 2: the library's bytes, batch by batch; every message on stderr"""
    net, lp = nets
    d = checkpoints
    frames = video_frames(71, 3, 34, 38, "nv12")
    (d / "in.yuv").write_bytes(frames.tobytes())
    run = _drive(d, "--size", "38x34", "--pix-fmt", "nv12", "--batch", "2", str(d / "in.yuv"), str(d / "out" / "out.yuv"))
    err = run.stderr.decode()
    print(err)
    assert run.returncode == 0, err
    assert run.stdout == b"" and err.rstrip("\n").split("\n")[-1] == f"3 frames -> {d / 'out' / 'out.yuv'}"
    fmt = Hn.VideoFormat("nv12", "bt601", False, "left")                                    # --matrix auto at 34 lines, the raw defaults
    want = torch.cat([Hn.enhance_yuv420(net, lp, cuda(frames[:2]), 34, 38, fmt), Hn.enhance_yuv420(net, lp, cuda(frames[2:]), 34, 38, fmt)])
    assert (d / "out" / "out.yuv").read_bytes() == host(want).tobytes()


def test_driver_y4m_stdin_to_stdout(Hn, nets, checkpoints):
    """two yuv420p10le frames as Y4M through pipes: the header line verbatim, FRAME before each frame, the library's bytes, nothing else"""
    net, lp = nets
    frames = video_frames(81, 2, 34, 38, "yuv420p10le")
    header = b"YUV4MPEG2 W38 H34 F25:1 Ip A1:1 C420p10 XYSCSS=420P10 XCOLORRANGE=LIMITED\n"
    stream = header + b"".join(b"FRAME\n" + f.astype("<u2").tobytes() for f in frames)
    run = _drive(checkpoints, "-", "-", stdin=stream)
    err = run.stderr.decode()
    print(err)
    assert run.returncode == 0, err
    assert err.rstrip("\n").split("\n")[-1] == "2 frames -> -"
    fmt = Hn.VideoFormat("yuv420p10le", "bt601", False, "left")
    want = host(Hn.enhance_yuv420(net, lp, cuda(frames), 34, 38, fmt))
    assert run.stdout == header + b"".join(b"FRAME\n" + f.astype("<u2").tobytes() for f in want)


def test_driver_refuses_a_stream_cut_mid_frame(Hn, nets, checkpoints):
    net, lp = nets
    d = checkpoints
    frames = video_frames(91, 2, 34, 38, "yuv420p")
    nbytes = frames.shape[1]
    (d / "cut.yuv").write_bytes(frames.tobytes()[:nbytes + 969])
    run = _drive(d, "--size", "38x34", str(d / "cut.yuv"), str(d / "cut_out.yuv"))
    err = run.stderr.decode()
    print(err)
    assert run.returncode not in (0, None) and run.returncode > 0 and run.stdout == b""
    assert f"969 of {nbytes} bytes" in err and "Traceback" not in err
    fmt = Hn.VideoFormat("yuv420p", "bt601", False, "left")
    assert (d / "cut_out.yuv").read_bytes() == host(Hn.enhance_yuv420(net, lp, cuda(frames[:1]), 34, 38, fmt)).tobytes()   # nothing partial
