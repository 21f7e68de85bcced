"""GPU: video evaluation from codec samples - fdn_yuv420_pair_stats / fdn_yuv420_ssim_y (include/fdn_vmetrics.h), fdn_hip.video_metrics
(pair_stats, ssim_y, VideoScore) and calculate_video_metrics.py, against the restatement of tests/vmetrics_ref.py.

Squared errors, luma sums, histograms, cut flags and dmean are integers (or one exactly formed quotient), so they are compared for
equality.  The luma SSIM is float64 from the codes on and is held to 1e-10 of the restatement, the bound the project holds fdn_ssim2d's
Y-plane SSIM to (tests/test_gpu_parity.py, tests/test_gpu_paired.py): each filtered quantity carries at most about 24 roundings of 2^-53
on magnitudes up to L^2, at most 3e-9 absolute at 10 bit, against denominators of at least C2 = 942, so the map's error is a few 1e-11 in
the worst case.

The kernel's tile is 32 x 32, so these are the smallest shapes at which it can go wrong (h x w, B):
  2x2, B=1     every tap of every window is a replicated sample; one chroma sample
  2x4, B=1     still all border
  12x14, B=1   the first size where a window lies wholly inside, plus a few more
  34x38, B=2   frame stride of 1938 samples: the second frame is not 16-byte aligned; two tiles on each axis
  70x514, B=2  3 x 17 tiles with partial last tiles; 32-bit partial sums would overflow at 10 bit
each over yuv420p, nv12 and yuv420p10le.
"""
import csv
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import vmetrics_ref as ref
from common import fdn_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fdn-tip2025_amd")
FMTS = list(ref.PIX_FMTS)
KINDS = ("random", "near", "identical", "extreme")

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


@pytest.fixture(scope="module")
def vm(Hn):
    from fdn_hip import video_metrics
    return video_metrics


def cuda(a):
    """numpy -> a contiguous tensor on the GPU; 16-bit samples travel as int16"""
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to("cuda:0").contiguous()


def fmt_of(Hn, pix):
    return Hn.VideoFormat(pix, "bt709", False, "left")


@functools.lru_cache(maxsize=None)
def inputs(shape, pix):
    """{kind: (a, b)} host frames of one shape and format, and the restatement's answers to them, computed once"""
    h, w, B = shape
    bits = ref.PIX_FMTS[pix][1]
    top = 2 ** bits - 1
    seed = 1000 * h + 10 * w + bits + (pix == "nv12")
    rng = np.random.default_rng(seed)
    a, b = ref.random_frames(seed, B, h, w, pix), ref.random_frames(seed + 1, B, h, w, pix)
    if bits == 10:                                           # some words above 1023, up to 0xFFFF
        for f in (a, b):
            k = max(1, f.size // 7)
            f.reshape(-1)[rng.choice(f.size, size=k, replace=False)] = rng.integers(1024, 0x10000, size=k)
        a.reshape(-1)[0], b.reshape(-1)[-1] = 0xFFFF, 0xFFFF
    legal = np.minimum(a, top)
    near = np.clip(legal.astype(np.int64) + rng.choice([-2, 2], size=a.shape), 0, top).astype(a.dtype)
    pairs = {"random": (a, b), "near": (legal, near), "identical": (a, a.copy()),
             "extreme": (np.zeros_like(a), np.full_like(a, top))}
    want = {k: (ref.pair_stats(x, y, h, w, pix), ref.ssim_y(x, y, h, w, pix)) for k, (x, y) in pairs.items()}
    return pairs, want


@pytest.mark.parametrize("pix", FMTS)
@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
def test_stats_and_ssim_against_the_restatement(Hn, vm, shape, pix):
    """pair_stats integer for integer, ssim_y within 1e-10, for random codes, b = a +- 2, b = a and 0 against the top code"""
    h, w, B = shape
    fmt = fmt_of(Hn, pix)
    pairs, want = inputs(shape, pix)
    for kind in KINDS:
        a, b = (cuda(x) for x in pairs[kind])
        stats = vm.pair_stats(a, b, h, w, fmt)
        assert stats.dtype == torch.int64 and stats.shape == (B, 5)
        assert [tuple(r) for r in stats.cpu().tolist()] == want[kind][0], kind
        ssim = vm.ssim_y(a, b, h, w, fmt)
        assert ssim.dtype == torch.float64 and ssim.shape == (B,)
        got = ssim.cpu().tolist()
        for t in range(B):
            print(f"{h}x{w} {pix} {kind} frame {t}: ssim {got[t]!r} restatement {want[kind][1][t]!r} diff {abs(got[t] - want[kind][1][t]):.3e}")
            assert abs(got[t] - want[kind][1][t]) <= 1e-10, (kind, t)
        alone = vm.pair_stats(a, None, h, w, fmt).cpu().tolist()
        assert [tuple(r) for r in alone] == [(0, 0, 0, s[3], 0) for s in want[kind][0]], kind
        if kind == "identical":
            assert all(abs(v - 1.0) <= 1e-10 for v in got)
            assert all(s[:3] == (0, 0, 0) and vm.psnr_from_sse(s[0], h * w, fmt.bits) == float("inf") for s in want[kind][0])
        if kind == "extreme":
            top = 2 ** fmt.bits - 1
            assert want[kind][0][0] == (top * top * h * w, top * top * h * w // 4, top * top * h * w // 4, 0, top * h * w)


@pytest.mark.parametrize("pix", FMTS)
@pytest.mark.parametrize("shape", ref.SHAPES[2:], ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
def test_ssim_against_fdn_ssim2d(Hn, vm, shape, pix):
    """the fused route against the existing one: fdn_ssim2d(replicate_no_crop=1, max_value=L) on the same luma as an fp32 plane (the codes
    are exact in fp32), frame by frame, within 2e-10: each is within 1e-10 of the float64 truth.  Every format and every kind of input.
    fdn_ssim2d refuses a side below 6 (FDN_ERR_ARG), so 2x2 and 2x4 have no counterpart there: they are held to the restatement alone."""
    from fdn_hip import metrics
    h, w, B = shape
    fmt = fmt_of(Hn, pix)
    pairs, _ = inputs(shape, pix)
    top = 2 ** fmt.bits - 1
    for kind in KINDS:
        a, b = pairs[kind]
        got = vm.ssim_y(cuda(a), cuda(b), h, w, fmt).cpu().tolist()
        ya, yb = ref.planes(a, h, w, pix)[0], ref.planes(b, h, w, pix)[0]
        for t in range(B):
            pa, pb = (torch.from_numpy(p[t].astype(np.float32)).to("cuda:0").reshape(1, h, w).contiguous() for p in (ya, yb))
            old = metrics._ssim2d(pa, pb, float(top), True)
            print(f"{h}x{w} {pix} {kind} frame {t}: fused {got[t]!r} fdn_ssim2d {old!r} diff {abs(got[t] - old):.3e}")
            assert abs(got[t] - old) <= 2e-10, (kind, t)


@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
def test_nv12_and_planar_frames_of_the_same_planes(Hn, vm, shape):
    """the same planes packed as yuv420p and as nv12: equal stats (the interleaved plane gives the two sums the planar planes give) and
    equal SSIM bits"""
    h, w, B = shape
    frames = ref.random_frames(77, B, h, w, "yuv420p")
    other = ref.random_frames(78, B, h, w, "yuv420p")
    as_nv12 = lambda f: ref.pack(*ref.unpack(f, h, w, "yuv420p"), "nv12")  # noqa: E731
    want = ref.pair_stats(frames, other, h, w, "yuv420p")
    assert want == ref.pair_stats(as_nv12(frames), as_nv12(other), h, w, "nv12") and want[0][1] != want[0][2]   # Cb and Cr can be told apart
    p = vm.pair_stats(cuda(frames), cuda(other), h, w, fmt_of(Hn, "yuv420p"))
    n = vm.pair_stats(cuda(as_nv12(frames)), cuda(as_nv12(other)), h, w, fmt_of(Hn, "nv12"))
    assert torch.equal(p, n) and [tuple(r) for r in n.cpu().tolist()] == want
    assert torch.equal(vm.ssim_y(cuda(frames), cuda(other), h, w, fmt_of(Hn, "yuv420p")),
                       vm.ssim_y(cuda(as_nv12(frames)), cuda(as_nv12(other)), h, w, fmt_of(Hn, "nv12")))


@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
def test_ten_bit_words_above_1023_count_as_1023(Hn, vm, shape):
    """a 10-bit frame and its copy clamped to 1023: equal stats, equal SSIM bits; int16 and uint16 tensors are the same frames"""
    h, w, B = shape
    fmt = fmt_of(Hn, "yuv420p10le")
    a, b = inputs(shape, "yuv420p10le")[0]["random"]
    assert a.max() > 1023 and b.max() > 1023
    ca, cb = np.minimum(a, 1023), np.minimum(b, 1023)
    assert torch.equal(vm.pair_stats(cuda(a), cuda(b), h, w, fmt), vm.pair_stats(cuda(ca), cuda(cb), h, w, fmt))
    raw, clamped = vm.ssim_y(cuda(a), cuda(b), h, w, fmt), vm.ssim_y(cuda(ca), cuda(cb), h, w, fmt)
    assert torch.equal(raw, clamped)
    assert torch.equal(vm.ssim_y(cuda(a).view(torch.uint16), cuda(b).view(torch.uint16), h, w, fmt), raw)
    assert torch.equal(vm.pair_stats(cuda(a).view(torch.uint16), None, h, w, fmt), vm.pair_stats(cuda(a), None, h, w, fmt))


@pytest.mark.parametrize("pix", FMTS)
@pytest.mark.parametrize("shape", [s for s in ref.SHAPES if s[2] > 1], ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
def test_ssim_bits_do_not_depend_on_slot_or_call(Hn, vm, shape, pix):
    """a frame pair in slot 0 and in slot 1 of a batch, and again in a second call: equal bits; both shapes that have a second slot"""
    h, w, _ = shape
    fmt = fmt_of(Hn, pix)
    a, b = inputs(shape, pix)[0]["random"]
    da, db = cuda(a), cuda(b)
    first = vm.ssim_y(da, db, h, w, fmt)
    swapped = vm.ssim_y(da.flip(0).contiguous(), db.flip(0).contiguous(), h, w, fmt)
    assert torch.equal(first, swapped.flip(0)) and first[0] != first[1]
    assert torch.equal(vm.ssim_y(da[1:].contiguous(), db[1:].contiguous(), h, w, fmt), first[1:])
    assert torch.equal(vm.ssim_y(da, db, h, w, fmt), first)
    assert torch.equal(vm.pair_stats(da, db, h, w, fmt), vm.pair_stats(da, db, h, w, fmt))


def same_records(got, want):
    """VideoScore's records against the restatement's: everything by equality but SSIM, which is held to 1e-10"""
    assert len(got) == len(want)
    for t, (g, r) in enumerate(zip(got, want)):
        assert set(g) == set(r)
        for k in r:
            if k == "ssim_y" and r[k] is not None:
                assert abs(g[k] - r[k]) <= 1e-10, (t, k, g[k], r[k])
            else:
                assert g[k] == r[k] and type(g[k]) is type(r[k]), (t, k, g[k], r[k])


@pytest.mark.parametrize("pix", FMTS)
def test_video_score_stream(Hn, vm, pix):
    """a 7-frame 34 x 38 stream whose content changes at frame 4: batches of 1, 3 and 7 give equal records, the cut flags are
    RatioFilter's, every record is the restatement's; with and without the reference"""
    from fdn_hip.temporal import RatioFilter
    h, w = 34, 38
    fmt = fmt_of(Hn, pix)
    r_host, d_host = ref.scene_stream(pix)
    want = ref.records(d_host, r_host, h, w, pix)
    assert [r["cut"] for r in want] == [True, False, False, False, True, False, False]
    assert all(r["dmean"] not in (None, 0.0) for r in want if not r["cut"])
    r_dev, d_dev = cuda(r_host), cuda(d_host)
    runs = {}
    for step in (1, 3, 7):
        s = vm.VideoScore(h, w, fmt, device="cuda:0")
        for i in range(0, 7, step):
            s.update(d_dev[i:i + step], r_dev[i:i + step])
        runs[step] = s
        same_records(s.frames, want)
        assert s.stats == ref.pair_stats(d_host, r_host, h, w, pix)
    assert runs[1].frames == runs[3].frames == runs[7].frames
    assert runs[1].summary() == runs[3].summary() == runs[7].summary()
    f = RatioFilter(h, w, fmt.bits, 1.0, cut=0.3, device="cuda:0")
    f.step(r_dev, torch.full((7, 1), 0.3, device="cuda:0"))
    assert [bool(c) for c in f.last_cut.cpu().tolist()] == [r["cut"] for r in runs[7].frames]
    out = runs[7].summary()
    fl = ref.flicker(want)
    assert (out["flicker"], out["flicker_ref"], out["flicker_err"]) == fl and min(fl) > 0 and out["cuts"] == 2 and out["frames"] == 7
    st = runs[7].stats
    assert out["psnr_y_global"] == ref.psnr(sum(x[0] for x in st), 7 * h * w, fmt.bits)
    assert out["psnr_avg_global"] == ref.psnr(sum(x[0] + x[1] + x[2] for x in st), 7 * h * w * 3 // 2, fmt.bits)
    # without a reference the stream's own content defines the scenes
    alone = vm.VideoScore(h, w, fmt, device="cuda:0")
    alone.update(d_dev[:3])
    alone.update(d_dev[3:])
    same_records(alone.frames, ref.records(d_host, None, h, w, pix))
    with pytest.raises(ValueError, match="reference"):
        alone.update(d_dev[:1], r_dev[:1])
    # the device argument: "cuda" takes frames of any ROCm device, an index only its own
    assert len(vm.VideoScore(h, w, fmt, device="cuda").update(d_dev[:1], r_dev[:1])) == 1
    with pytest.raises(Hn.FdnHipError, match="cuda:1"):
        vm.VideoScore(h, w, fmt, device="cuda:1").update(d_dev[:1], r_dev[:1])


def test_flicker_end_to_end(Hn, vm):
    """four identical dim 34 x 38 frames through enhance_yuv420(ratio_mode="fixed"): a constant ratio gives identical outputs and
    flicker == 0.0 exactly, a ratio alternating between two values gives flicker > 0 (the input, which does not change, is the
    reference and defines the scenes).  The tamed weights answer the ratio only faintly - in the float64-checked CPU oracle the luma
    of this frame sums to 115,969.49 codes before rounding at ratio 0.3 and to 115,936.46 at 300, and 0.3 against 0.45 moves it by 1e-4 -
    so the two values lie far apart: 33 codes over 1,292 pixels is what has to show in the 8-bit output."""
    from basicsr.models.archs.FDN_arch import FDN
    net = FDN()
    net.load_state_dict(fdn_weights(tame=0.03), strict=True)
    net = net.to("cuda:0").eval()
    h, w = 34, 38
    fmt = Hn.VideoFormat("yuv420p", "bt601", False, "left")
    frames = cuda(np.repeat(ref.random_frames(5, 1, h, w, "yuv420p", lo=16, hi=60), 4, axis=0))
    figures = {}
    for name, ratio in (("constant", [0.3] * 4), ("alternating", [0.3, 300.0, 0.3, 300.0])):
        out = Hn.enhance_yuv420(net, None, frames, h, w, fmt, ratio_mode="fixed", ratio=torch.tensor(ratio, device="cuda:0").reshape(4, 1))
        s = vm.VideoScore(h, w, fmt, device="cuda:0")
        s.update(out, frames)
        assert [r["cut"] for r in s.frames] == [True, False, False, False]
        figures[name] = s.summary()
        print(name, [r["mean_y"] for r in s.frames], figures[name]["flicker"])
    assert figures["constant"]["flicker"] == 0.0 and figures["constant"]["flicker_ref"] == 0.0
    assert figures["alternating"]["flicker"] > 0 and figures["alternating"]["flicker_ref"] == 0.0
    assert figures["alternating"]["flicker_err"] == figures["alternating"]["flicker"]


def y4m(frames, w=38, h=34):
    return b"YUV4MPEG2 W%d H%d F25:1 Ip A1:1 C420p10\n" % (w, h) + b"".join(b"FRAME\n" + f.astype("<u2").tobytes() for f in frames)


def read_csv(path):
    rows = list(csv.reader(open(path)))
    assert rows[0] == ["frame", "psnr_y", "psnr_u", "psnr_v", "psnr_avg", "ssim_y", "mean_y_ref", "mean_y", "cut", "dmean_ref", "dmean"]
    out = []
    for n, row in enumerate(rows[1:]):
        rec = dict(zip(rows[0], row))
        assert int(rec.pop("frame")) == n
        out.append({k: (bool(int(v)) if k == "cut" else None if v == "" else float(v)) for k, v in rec.items()})
    return out


def test_tool(Hn, vm, tmp_path):
    """calculate_video_metrics.py on two 3-frame 10-bit Y4M streams: file to file and DIST through stdin give VideoScore's records back
    exactly (floats written with repr), exit status 0, messages on stderr; REF one frame longer: the common prefix, both lengths, status 1"""
    h, w, pix = 34, 38, "yuv420p10le"
    r_host, d_host = ref.scene_stream(pix, n=4, change_at=2)
    (tmp_path / "ref.y4m").write_bytes(y4m(r_host[:3]))
    (tmp_path / "dist.y4m").write_bytes(y4m(d_host[:3]))
    (tmp_path / "long.y4m").write_bytes(y4m(r_host))
    s = vm.VideoScore(h, w, Hn.VideoFormat(pix, "bt601", False, "left"), device="cuda:0")
    s.update(cuda(d_host[:3]), cuda(r_host[:3]))
    assert [r["cut"] for r in s.frames] == [True, False, True]
    tool = [sys.executable, os.path.join(PKG, "calculate_video_metrics.py"), "--batch", "2"]

    def run(args, **kw):
        p = subprocess.run(tool + args, capture_output=True, timeout=600, **kw)
        print(p.stderr.decode())
        return p, p.stdout.decode().rstrip("\n").split("\n"), p.stderr.decode()

    p, lines, err = run(["--ref", str(tmp_path / "ref.y4m"), str(tmp_path / "dist.y4m"), "--csv", str(tmp_path / "a.csv")])
    assert p.returncode == 0, err
    assert read_csv(tmp_path / "a.csv") == s.frames
    assert len(lines) == 5 and lines[3].startswith("Average:") and lines[4].startswith("flicker:") and all(":" in x for x in lines[:3])
    assert "3 frames scored" in err and "Traceback" not in err
    p, lines2, err = run(["--ref", str(tmp_path / "ref.y4m"), "-", "--csv", str(tmp_path / "b.csv")], input=y4m(d_host[:3]))
    assert p.returncode == 0, err
    assert (tmp_path / "b.csv").read_bytes() == (tmp_path / "a.csv").read_bytes() and lines2 == lines
    p, lines3, err = run(["--ref", str(tmp_path / "long.y4m"), str(tmp_path / "dist.y4m"), "--csv", str(tmp_path / "c.csv")])
    assert p.returncode == 1 and "Traceback" not in err
    last = err.rstrip("\n").split("\n")[-1]
    assert "has 4 frames" in last and "has 3" in last and "first 3" in last
    assert read_csv(tmp_path / "c.csv") == s.frames and lines3[:3] == lines[:3]
    # without --ref: mean_y, cut, dmean and flicker only
    p, lines4, err = run([str(tmp_path / "dist.y4m")])
    assert p.returncode == 0 and len(lines4) == 5 and "PSNR" not in "".join(lines4) and "SSIM" not in "".join(lines4)
    assert all("mean_y" in x and "cut" in x and "dmean" in x for x in lines4[:3]) and lines4[4].startswith("flicker:")
