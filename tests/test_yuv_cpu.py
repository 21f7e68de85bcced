"""CPU: the host side of the video route - the entry points of include/fdn_video.h (versions, prototype table, argument checks before any
launch), the Y4M / raw stream handling of inference_fdn_video.py, the float64 restatement of tests/yuv_ref.py judged on its own, and
the checks fdn_hip.harness.enhance_yuv420 makes before anything runs.  No GPU compute."""
import ctypes
import io
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as entry  # noqa: F401  (puts the package on sys.path)
import yuv_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import fdn_hip
    if not os.path.isfile(fdn_hip.lib_path()):
        entry.build()
    return fdn_hip.lib()


def test_versions_and_prototype_tables(lib):
    """the entry points of include/fdn_video.h in the one table (tests/test_host_cpu.py holds it to the headers): names, signatures"""
    from fdn_hip._abi import HEADERS, PROTOTYPES
    assert HEADERS["fdn_video.h"] == ["fdn_video_abi_version", "fdn_pre_yuv420", "fdn_post_yuv420"]
    assert PROTOTYPES["fdn_pre_yuv420"] == PROTOTYPES["fdn_post_yuv420"] == ("I", ["P", "P"] + ["I"] * 10 + ["P"])
    assert lib.fdn_pre_yuv420.argtypes == [ctypes.c_void_p] * 2 + [ctypes.c_int] * 10 + [ctypes.c_void_p]


def test_entry_points_validate_arguments_without_gpu(lib):
    """every refusal of include/fdn_video.h returns FDN_ERR_ARG = 1 before any launch, for both entry points"""
    p = ctypes.c_void_p(64)                          # never dereferenced: every call below fails its argument check
    for f, pre in ((lib.fdn_pre_yuv420, True), (lib.fdn_post_yuv420, False)):
        def call(a=p, b=p, B=1, h=34, w=38, H=64, W=64, layout=0, bits=8, matrix=0, full_range=0, chroma_loc=0):
            return f(a, b, B, h, w, H, W, layout, bits, matrix, full_range, chroma_loc, None)
        assert call(a=None) == 1 and call(b=None) == 1
        assert call(h=33) == 1 and call(w=37) == 1 and call(h=0) == 1 and call(w=0) == 1 and call(h=-2) == 1
        assert call(bits=9) == 1 and call(bits=12) == 1 and call(bits=16) == 1 and call(bits=0) == 1
        assert call(layout=1, bits=10) == 1 and call(layout=2) == 1 and call(layout=-1) == 1
        for key in ("matrix", "full_range", "chroma_loc"):
            assert call(**{key: 2}) == 1 and call(**{key: -1}) == 1, key
        assert call(H=32) == 1 and call(W=36) == 1                                          # H < h, W < w
        assert call(B=0) == 1 and call(B=65536) == 1
        if pre:
            assert call(H=68) == 1 and call(W=76) == 1 and call(h=2, w=2, H=4, W=2) == 1   # reflect padding: pad >= size
            assert call(h=65536, H=65536) == 1 and call(h=65534, H=65536) == 1              # grid.y = H
        else:
            assert call(h=65536, H=65536) == 1                                              # as fdn_post_u8: h < 65536


def _driver():
    import inference_fdn_video
    return inference_fdn_video


def test_y4m_header_tags():
    drv = _driver()
    for tag, want in (("C420jpeg", ("yuv420p", "center")), ("C420", ("yuv420p", "center")), (None, ("yuv420p", "center")),
                      ("C420mpeg2", ("yuv420p", "left")), ("C420p10", ("yuv420p10le", "left"))):
        line = b"YUV4MPEG2 W38 H34 F25:1 Ip A1:1" + (b" " + tag.encode() if tag else b"") + b"\n"
        hdr = drv.parse_y4m_header(line)
        assert (hdr.pix_fmt, hdr.chroma_loc) == want and (hdr.width, hdr.height, hdr.full_range) == (38, 34, None), tag
        assert hdr.line == line                                                             # written back verbatim
        fmt = drv.y4m_format(hdr)
        assert (fmt.pix_fmt, fmt.chroma_loc, fmt.full_range, fmt.matrix) == (*want, False, "bt601")
    for tag in ("C420paldv", "C422", "C444", "Cmono", "C420p12", "C422p10", "C444alpha"):
        with pytest.raises(ValueError, match=tag + r"\b"):
            drv.parse_y4m_header(b"YUV4MPEG2 W38 H34 F25:1 Ip " + tag.encode() + b"\n")
    for flag in ("It", "Ib", "Im"):
        with pytest.raises(ValueError, match=flag):
            drv.parse_y4m_header(b"YUV4MPEG2 W38 H34 " + flag.encode() + b" C420mpeg2\n")
    assert drv.parse_y4m_header(b"YUV4MPEG2 W38 H34 I? C420mpeg2\n").chroma_loc == "left"
    for bad in (b"YUV4MPEG2 W38 C420\n", b"YUV4MPEG2 H34\n", b"YUV4MPEG2 W37 H34\n", b"YUV4MPEG W38 H34\n", b"P6\n38 34\n"):
        with pytest.raises(ValueError):
            drv.parse_y4m_header(bad)


def test_y4m_colour_range_and_overrides():
    drv = _driver()
    base = b"YUV4MPEG2 W1280 H720 F30:1 Ip A1:1 C420p10 XYSCSS=420P10"
    assert drv.parse_y4m_header(base + b"\n").full_range is None
    full = drv.parse_y4m_header(base + b" XCOLORRANGE=FULL\n")
    lim = drv.parse_y4m_header(base + b" XCOLORRANGE=LIMITED\n")
    assert full.full_range is True and lim.full_range is False
    assert drv.y4m_format(full).full_range is True and drv.y4m_format(lim).full_range is False
    with pytest.raises(ValueError, match="XCOLORRANGE"):
        drv.parse_y4m_header(base + b" XCOLORRANGE=WIDE\n")
    fmt = drv.y4m_format(full)
    assert (fmt.pix_fmt, fmt.matrix, fmt.chroma_loc, fmt.bits, fmt.layout) == ("yuv420p10le", "bt709", "left", 10, 0)
    # explicit flags beat the header
    fmt = drv.y4m_format(full, matrix="bt601", full_range=False, chroma_loc="center")
    assert (fmt.matrix, fmt.full_range, fmt.chroma_loc) == ("bt601", False, "center")
    hdr8 = drv.parse_y4m_header(b"YUV4MPEG2 W38 H34 C420jpeg\n")
    assert drv.y4m_format(hdr8, pix_fmt="nv12").layout == 1


def test_matrix_auto_rule():
    drv = _driver()
    assert drv.auto_matrix(576) == "bt601" and drv.auto_matrix(578) == "bt709"
    assert drv.auto_matrix(480) == "bt601" and drv.auto_matrix(720) == "bt709"
    assert drv.video_format(576).matrix == "bt601" and drv.video_format(578).matrix == "bt709"
    assert drv.video_format(576, matrix="bt709").matrix == "bt709"


def test_frame_bytes_and_video_format():
    drv = _driver()
    from fdn_hip import FdnHipError
    from fdn_hip.harness import VideoFormat
    assert drv.frame_bytes("yuv420p", 38, 34) == drv.frame_bytes("nv12", 38, 34) == 38 * 34 * 3 // 2 == 1938
    assert drv.frame_bytes("yuv420p10le", 38, 34) == 3876
    assert drv.frame_bytes("yuv420p", 1280, 720) == 1382400 and drv.frame_bytes("yuv420p10le", 1280, 720) == 2764800
    for bad in (("yuv420p", 37, 34), ("yuv420p", 38, 33), ("yuv420p", 0, 34), ("yuv422p", 38, 34)):
        with pytest.raises(ValueError):
            drv.frame_bytes(*bad)
    for pix, layout, bits, dtype in (("yuv420p", 0, 8, torch.uint8), ("nv12", 1, 8, torch.uint8), ("yuv420p10le", 0, 10, torch.int16)):
        fmt = VideoFormat(pix)
        assert (fmt.layout, fmt.bits, fmt.dtype, fmt.frame_samples(34, 38)) == (layout, bits, dtype, 1938)
        assert fmt.frame_samples(34, 38) * fmt.sample_bytes == drv.frame_bytes(pix, 38, 34)
        assert (fmt.matrix, fmt.full_range, fmt.chroma_loc) == ("bt709", False, "left")
        with pytest.raises(FdnHipError):
            fmt.frame_samples(33, 38)
    for kw in (dict(pix_fmt="p010le"), dict(matrix="bt2020"), dict(chroma_loc="topleft")):
        with pytest.raises(ValueError):
            VideoFormat(**kw)


@pytest.mark.parametrize("y4m", [False, True], ids=["raw", "y4m"])
def test_reader_batches_and_refuses_a_stream_cut_mid_frame(y4m):
    drv = _driver()
    nbytes = drv.frame_bytes("yuv420p", 4, 2)
    frames = np.arange(5 * nbytes, dtype=np.uint8).reshape(5, nbytes)
    body = b"".join((b"FRAME\n" if y4m else b"") + f.tobytes() for f in frames)

    def reader(data, prefix=0):
        return drv.FrameReader(io.BytesIO(data[prefix:]), nbytes, y4m, prefix=data[:prefix])
    # whole stream, a short last batch, then a clean end; bytes already taken from the stream come first
    for prefix in (0, 10):
        r = reader(body, prefix)
        buf = np.zeros((2, nbytes), dtype=np.uint8)
        got = []
        while True:
            n = r.read_batch(buf)
            got += [buf[i].copy() for i in range(n)]
            if n < 2:
                break
        assert len(got) == 5 == r.frames and np.array_equal(np.stack(got), frames) and r.error is None
        assert r.read_batch(buf) == 0
    # cut inside the fourth frame: three complete frames come out, nothing of the fourth, and the next call refuses
    cut = len(body) - (len(body) // 5) - 5                                     # the last frame and 5 bytes of the one before
    r = reader(body[:cut])
    buf = np.zeros((8, nbytes), dtype=np.uint8)
    assert r.read_batch(buf) == 3 and np.array_equal(buf[:3], frames[:3])
    assert r.error is not None and f"{nbytes - 5} of {nbytes} bytes" in r.error
    with pytest.raises(drv.TruncatedInput, match=f"{nbytes - 5} of {nbytes}"):
        r.read_batch(buf)
    out = io.BytesIO()
    drv.write_frames(out, frames, y4m)
    assert out.getvalue() == body


def test_restatement_grey_is_grey_and_round_trips():
    """neutral chroma gives R = G = B; over all legal grey codes post64(pre64(.)) is the identity, at 8 and 10 bit, every format"""
    for pix, m, full, loc in ref.FORMATS:
        bits = ref.PIX_FMTS[pix][1]
        s = 2 ** (bits - 8)
        codes = np.arange(16 * s, 235 * s + 1)
        if full:
            codes = np.arange(0, 2 ** bits)
        w = 2 * ((len(codes) + 1) // 2)
        y = np.resize(codes, (1, 2, w))
        c = np.full((1, 1, w // 2), 128 * s)
        frames = ref.pack(y, c, c, pix)
        x = ref.pre64(frames, 2, w, 2, w, pix, m, full, loc)
        assert np.array_equal(x[:, 0], x[:, 1]) and np.array_equal(x[:, 1], x[:, 2])
        assert x.min() == 0.0 and x.max() == 1.0
        back, exact = ref.post64(x, 2, w, pix, m, full, loc)
        assert back.dtype == frames.dtype and np.array_equal(back, frames), (pix, m, full, loc)
        assert np.abs(exact - frames).max() < 1e-9


def test_restatement_pads_by_reflection_and_clamps():
    frames = ref.random_frames(5, 1, 18, 22, "yuv420p")
    for loc in ("left", "center"):
        x = ref.pre64(frames, 18, 22, 32, 32, "yuv420p", "bt709", False, loc)
        assert x.shape == (1, 3, 32, 32) and x.min() >= 0.0 and x.max() <= 1.0 and x.min() == 0.0 and x.max() == 1.0
        assert np.array_equal(x[:, :, 18:], x[:, :, 16:2:-1]) and np.array_equal(x[:, :, :, 22:], x[:, :, :, 20:10:-1])
        assert np.array_equal(x[:, :, :18, :22], ref.pre64(frames, 18, 22, 18, 22, "yuv420p", "bt709", False, loc))
    # a constant chroma plane interpolates to itself; nv12 and yuv420p hold the same planes
    y, u, v = ref.unpack(frames, 18, 22, "yuv420p")
    assert np.array_equal(ref.pre64(ref.pack(y, u, v, "nv12"), 18, 22, 18, 22, "nv12", "bt601", True, "left"),
                          ref.pre64(frames, 18, 22, 18, 22, "yuv420p", "bt601", True, "left"))
    # a 10-bit word above 1023 counts as 1023
    big = np.full((1, 6), 0xFFFF, dtype=np.uint16)
    assert np.array_equal(ref.pre64(big, 2, 2, 2, 2, "yuv420p10le", "bt709", True, "left"),
                          ref.pre64(np.full((1, 6), 1023, dtype=np.uint16), 2, 2, 2, 2, "yuv420p10le", "bt709", True, "left"))


def test_restatement_post_never_reads_the_padding():
    res = ref.random_planes(3, 1, 32, 32)
    want = ref.post64(res, 18, 22, "yuv420p", "bt709", False, "left")[0]
    res[:, :, 18:] = 9.0
    res[:, :, :, 22:] = -9.0
    assert np.array_equal(ref.post64(res, 18, 22, "yuv420p", "bt709", False, "left")[0], want)


def test_near_tie_share_of_the_gpu_cases():
    """for every case of tests/test_gpu_yuv.py's post test, under 1 % of the samples lie within 1e-3 code units of a rounding tie (a
    property of the seeded inputs and the restatement alone)"""
    worst = 0.0
    for h, w, H, W, B in ref.SHAPES:
        res = ref.random_planes(ref.POST_SEED, B, H, W)
        for pix, m, full, loc in ref.FORMATS:
            exact = ref.post64(res, h, w, pix, m, full, loc)[1]
            share = float(ref.near_tie(exact).mean())
            worst = max(worst, share)
            assert share < 0.01, (h, w, pix, m, full, loc, share)
    print(f"largest near-tie share {100 * worst:.3f} %")


def test_enhance_yuv420_checks_before_anything_runs(lib):
    import inspect
    from fdn_hip import FdnHipError, harness
    fmt8, fmt10 = harness.VideoFormat("yuv420p"), harness.VideoFormat("yuv420p10le")
    assert inspect.signature(harness.enhance_yuv420).parameters["blend"].default == "average"
    n = fmt8.frame_samples(34, 38)
    good8, good10 = torch.zeros(2, n, dtype=torch.uint8), torch.zeros(2, n, dtype=torch.int16)
    for frames, fmt in ((good8.to(torch.int16), fmt8), (good8.float(), fmt8), (good10.to(torch.uint8), fmt10), (good10.to(torch.int32), fmt10)):
        with pytest.raises(FdnHipError, match="frames must be"):
            harness.enhance_yuv420(None, None, frames, 34, 38, fmt)
    for frames in (good8[:, :-1], torch.zeros(2, 34, 38, dtype=torch.uint8), torch.zeros(2, n * 2, dtype=torch.uint8)):
        with pytest.raises(FdnHipError, match="expected yuv420p frames"):
            harness.enhance_yuv420(None, None, frames, 34, 38, fmt8)
    with pytest.raises(FdnHipError, match="even"):
        harness.enhance_yuv420(None, None, good8, 33, 38, fmt8)
    for bad in ("linear", "Feather", None):
        with pytest.raises(ValueError, match="blend"):
            harness.enhance_yuv420(None, None, good8, 34, 38, fmt8, blend=bad)
        with pytest.raises(ValueError, match="blend"):
            harness.enhance_yuv420(None, None, good8, 34, 38, fmt8, tile=(32, 32), blend=bad)
    with pytest.raises(ValueError, match="ratio_mode"):
        harness.enhance_yuv420(None, None, good8, 34, 38, fmt8, ratio_mode="gt")
    # no host fallback: well-formed frames on the CPU are refused too
    for frames, fmt in ((good8, fmt8), (good10, fmt10), (good10.view(torch.uint16), fmt10)):
        with pytest.raises(FdnHipError, match="ROCm"):
            harness.enhance_yuv420(None, None, frames, 34, 38, fmt)
    with pytest.raises(FdnHipError, match="ROCm"):
        harness.postprocess_yuv420(torch.zeros(1, 3, 64, 64), 34, 38, fmt8)


def test_tile_ratio_still_checks_its_arguments():
    """tile_ratio keeps its signature and its refusals after its frame branch was factored out"""
    import inspect
    from fdn_hip import FdnHipError, harness
    assert list(inspect.signature(harness.tile_ratio).parameters) == ["lpnet", "img_u8", "tiles", "ratio_mode", "ratio_from", "bgr", "ratio",
                                                                      "gt_u8", "batch"]
    tiles, img = torch.zeros(4, 3, 32, 32), torch.zeros(64, 64, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="ratio_from"):
        harness.tile_ratio(None, img, tiles, "lolblur", "pixel")
    with pytest.raises(FdnHipError, match="needs lpnet"):
        harness.tile_ratio(None, img, tiles, "lolblur", "frame")
    with pytest.raises(FdnHipError, match="ground-truth"):
        harness.tile_ratio(None, img, tiles, "gt", "frame")
    r = harness.tile_ratio(None, img, tiles, "fixed", "tile", ratio=torch.tensor([[2.0]]))
    assert r.shape == (4, 1) and r.is_contiguous() and float(r.min()) == 2.0
