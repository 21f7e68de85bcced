"""GPU: motion-compensated temporal consistency (include/fdn_motion.h, libfdn_motion.so, fdn_hip.motion) against the numpy restatement of
tests/motion_ref.py.  Every quantity is an integer, so every comparison is for equality; only the formatted floats of the tool are compared
as text.

Shapes h x w, B, R - the smallest at which a 16 x 16 block kernel with a clamped window can go wrong:
    2 x 2,    B 2, R 8     one partial block, every window sample a clamp (and most candidates tie)
    16 x 16,  B 2, R 16    one full block, the window wholly outside it
    18 x 34,  B 3, R 1     2 x 3 blocks, a 2-pixel partial row and column
    34 x 50,  B 3, R 8     partial last blocks, an odd frame stride (2550 samples: frames are not 16-byte aligned)
    70 x 130, B 2, R 16    5 x 9 blocks, the largest window
    34 x 50,  B 2, R 0     the search degenerates to the zero vector
each over yuv420p, nv12 and yuv420p10le, with 10-bit words above 1023 among the samples.  Data: random frames; a known shift; stripes of
period 4 (ties); identical frames; "extreme" (guide 0 then top, dist top then 0: rD - rG = +-2 top in every pixel, where a signed 32-bit
partial over more than two blocks overflows); guide is dist."""
import csv
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import motion_ref as ref
from test_motion_cpu import check_argument_errors

from common import poison_uninitialized  # noqa: F401  (autouse, tests/common.py: torch.empty is filled with NaN / the integer maximum)
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fdn-tip2025_amd")
PIXES = ["yuv420p", "nv12", "yuv420p10le"]


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import fdn_hip
    fdn_hip.lib()   # fail loudly if the HIP extension is not built
    from fdn_hip import motion
    motion.lib()
    return motion


@pytest.fixture(scope="module")
def Hn(M):
    from fdn_hip import harness
    return harness


def cuda(a):
    """numpy -> a contiguous tensor on the GPU; 16-bit samples travel as int16"""
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to("cuda:0").contiguous()


def fmt_of(Hn, pix):
    return Hn.VideoFormat(pix, "bt709", False, "left")


def host(t):
    return t.cpu().numpy().astype(np.int64)


@functools.lru_cache(maxsize=None)
def random_case(shape, pix):
    """host frames of one shape and format - a guide batch, a scored batch and the one frame before each - and the restatement's answers,
    computed once"""
    h, w, B, R = shape
    seed = 1000 * h + 10 * w + len(pix)
    g, d = ref.frames_of(ref.random_lumas(B + 1, h, w, pix, seed), pix, seed), ref.frames_of(ref.random_lumas(B + 1, h, w, pix, seed + 1), pix, seed + 1)
    mv, sad, ss = ref.search(g[1:], g[0], h, w, pix, R)
    rs = ref.residual(d[1:], d[0], g[1:], g[0], mv, h, w, pix)
    return g, d, mv, sad, ss, rs


def run(M, Hn, pix, h, w, R, g, gp, d=None, dp=None):
    """search on g, residual of d (default: g itself) -> host (mv, sad, search stats, residual stats)"""
    fmt = fmt_of(Hn, pix)
    tg, tgp = cuda(g), (None if gp is None else cuda(gp))
    mv, sad, ss = M.search(tg, tgp, h, w, fmt, radius=R)
    if d is None:
        rs = M.residual(tg, tgp, tg, tgp, mv, h, w, fmt)
    else:
        rs = M.residual(cuda(d), None if dp is None else cuda(dp), tg, tgp, mv, h, w, fmt)
    assert mv.dtype == torch.int16 and sad.dtype == torch.int32 and sad.view(torch.int64).shape == (*sad.shape[:-1], 1)
    return host(mv), host(sad), [tuple(r) for r in ss.cpu().tolist()], [tuple(r) for r in rs.cpu().tolist()]


# ---------------------------------------------------------------------------------------------------------------------------------
# random frames at every shape and format
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pix", PIXES)
@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: "%dx%d-B%d-R%d" % s)
def test_random_frames_equal_restatement(M, Hn, shape, pix):
    h, w, B, R = shape
    g, d, want_mv, want_sad, want_ss, want_rs = random_case(shape, pix)
    if ref.PIX_FMTS[pix][1] == 10 and h * w >= 256:
        assert (g[:, :h * w] > 1023).any() and (d[:, :h * w] > 1023).any()             # words above the top code are among the samples
    mv, sad, ss, rs = run(M, Hn, pix, h, w, R, g[1:], g[0], d[1:], d[0])
    assert np.array_equal(mv, want_mv) and np.array_equal(sad, want_sad) and ss == want_ss and rs == want_rs
    assert ss == [(int(sad[i, ..., 0].sum()), int(sad[i, ..., 1].sum()), int(np.abs(mv[i]).sum()), int((mv[i] != 0).any(-1).sum())) for i in range(B)]
    if R == 0:
        assert not mv.any() and np.array_equal(sad[..., 0], sad[..., 1])
    # the frame before left out: frame 0's rows are 0, the others are what they were
    mv0, sad0, ss0, rs0 = run(M, Hn, pix, h, w, R, g[1:], None, d[1:], None)
    assert not mv0[0].any() and not sad0[0].any() and ss0[0] == (0, 0, 0, 0) and rs0[0] == (0, 0, 0, 0, 0)
    assert np.array_equal(mv0[1:], want_mv[1:]) and np.array_equal(sad0[1:], want_sad[1:]) and ss0[1:] == want_ss[1:] and rs0[1:] == want_rs[1:]
    # the guide scored against itself: words 2 - 3 repeat words 0 - 1, word 4 is 0, and sum |rG| is the sum of the chosen SADs
    _, _, ss1, rs1 = run(M, Hn, pix, h, w, R, g[1:], g[0])
    assert ss1 == want_ss and all(r[2:4] == r[0:2] and r[4] == 0 and r[0] == s[0] and r[2:4] == q[2:4] for r, s, q in zip(rs1, ss1, want_rs))


@pytest.mark.parametrize("pix", PIXES)
def test_batches_carry_the_frame_before(M, Hn, pix):
    """a batch of 3 equals batches of 1 + 2 with the carried frame"""
    shape = (34, 50, 3, 8)
    h, w, B, R = shape
    g, d, want_mv, want_sad, want_ss, want_rs = random_case(shape, pix)
    a = run(M, Hn, pix, h, w, R, g[1:2], g[0], d[1:2], d[0])
    b = run(M, Hn, pix, h, w, R, g[2:], g[1], d[2:], d[1])
    assert np.array_equal(np.concatenate([a[0], b[0]]), want_mv) and np.array_equal(np.concatenate([a[1], b[1]]), want_sad)
    assert a[2] + b[2] == want_ss and a[3] + b[3] == want_rs


@pytest.mark.parametrize("pix", PIXES)
def test_outputs_not_wanted_and_argument_errors(M, Hn, pix):
    """mv = NULL / sad = NULL give the same stats and write nothing else; the refusals of the CPU test hold with a device present"""
    import ctypes
    shape = (34, 50, 3, 8)
    h, w, B, R = shape
    g, _, want_mv, want_sad, want_ss, _ = random_case(shape, pix)
    tg, tp = cuda(g[1:]), cuda(g[0])
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    bits = ref.PIX_FMTS[pix][1]
    for with_mv, with_sad in ((False, False), (True, False), (False, True)):
        mv = torch.full((B, 3, 4, 2), 77, dtype=torch.int16, device="cuda:0")
        sad = torch.full((B, 3, 4, 2), 77, dtype=torch.int32, device="cuda:0")
        stats = torch.full((B, 4), 77, dtype=torch.int64, device="cuda:0")           # cleared by the call, not by the caller
        rc = M.lib().fdn_motion_search(p(tg), p(tp), p(mv) if with_mv else None, p(sad) if with_sad else None, p(stats), B, h, w, bits, R, None)
        torch.cuda.synchronize()
        assert rc == 0 and [tuple(r) for r in stats.cpu().tolist()] == want_ss
        assert np.array_equal(host(mv), want_mv) if with_mv else (mv == 77).all()
        assert np.array_equal(host(sad), want_sad) if with_sad else (sad == 77).all()
    check_argument_errors(M.lib())


# ---------------------------------------------------------------------------------------------------------------------------------
# data with a known answer
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pix", PIXES)
def test_known_shift(M, Hn, pix):
    """content moving by (-3, +5) per frame: (3, -5) with SAD 0 wherever the match lies inside the frame, then everything against the
    restatement"""
    h, w, R = 70, 130, 8
    g = ref.frames_of(ref.shifted_stream(3, h, w, pix, (-3, 5), seed=11), pix)
    mv, sad, ss, rs = run(M, Hn, pix, h, w, R, g, None)
    assert (mv[1:, :-1, 1:] == (3, -5)).all() and not sad[1:, :-1, 1:, 0].any() and sad[1:, :-1, 1:, 1].all()
    want_mv, want_sad, want_ss = ref.search(g, None, h, w, pix, R)
    assert np.array_equal(mv, want_mv) and np.array_equal(sad, want_sad) and ss == want_ss
    assert rs == ref.residual(g, None, g, None, want_mv, h, w, pix)


@pytest.mark.parametrize("pix", PIXES)
def test_stripes_and_identical_frames(M, Hn, pix):
    """stripes of period 4: candidates 4 columns apart, and every dy, cost the same; the shortest wins, then the smaller dy, then dx"""
    h, w, R = 34, 70, 8
    still = ref.frames_of(ref.stripes(2, h, w, pix, move=0), pix)
    mv, sad, ss, rs = run(M, Hn, pix, h, w, R, still, None)
    assert not mv.any() and not sad.any() and ss == [(0, 0, 0, 0)] * 2 and rs == [(0, 0, 0, 0, 0)] * 2
    moved = ref.frames_of(ref.stripes(3, h, w, pix, move=1), pix)
    mv, sad, ss, rs = run(M, Hn, pix, h, w, R, moved, None)
    assert (mv[1:, :, 1:-1] == (0, -1)).all() and not sad[1:, :, 1:-1, 0].any()
    want_mv, want_sad, want_ss = ref.search(moved, None, h, w, pix, R)
    assert np.array_equal(mv, want_mv) and np.array_equal(sad, want_sad) and ss == want_ss
    same = ref.frames_of(np.repeat(ref.random_lumas(1, 34, 50, pix, 5), 3, axis=0), pix)
    mv, sad, ss, rs = run(M, Hn, pix, 34, 50, 16, same, same[0])
    assert not mv.any() and not sad.any() and ss == [(0, 0, 0, 0)] * 3 and rs == [(0, 0, 0, 0, 0)] * 3


@pytest.mark.parametrize("pix", PIXES)
def test_extreme_values(M, Hn, pix):
    """guide 0 then top, dist top then 0: the zero vector everywhere (every candidate costs the same), rD = -top, rG = top, and rD - rG =
    -2 top in every pixel.  At 10 bit a full block's sum of squares is 256 * 2046^2 = 1 071 645 696 (just below 2^30), the
    sum over the 64 x 16 pixels a workgroup of the residual kernel walks at a time 4 286 582 784, beyond a signed 32-bit partial and 0.2 %
    short of an unsigned one, and the frame's beyond both"""
    h, w, R = 34, 50, 8
    top, n = ref.top_of(pix), h * w
    raw_top = 65535 if ref.PIX_FMTS[pix][1] == 10 else top                               # 10 bit: written as a word above 1023
    g = ref.frames_of(np.stack([np.zeros((h, w), dtype=np.int64), np.full((h, w), raw_top)]), pix)
    d = ref.frames_of(np.stack([np.full((h, w), raw_top), np.zeros((h, w), dtype=np.int64)]), pix)
    mv, sad, ss, rs = run(M, Hn, pix, h, w, R, g, None, d, None)
    assert not mv.any() and (sad[1, 0, 0] == 256 * top).all() and ss[1] == (n * top, n * top, 0, 0)
    assert rs[1] == (n * top, n * top * top, n * top, n * top * top, n * 4 * top * top)
    assert rs == ref.residual(d, None, g, None, mv, h, w, pix)
    if top == 1023:
        assert 256 * (2 * top) ** 2 < 2 ** 30 and 2 ** 31 < 1024 * (2 * top) ** 2 < 2 ** 32 < rs[1][4]


# ---------------------------------------------------------------------------------------------------------------------------------
# MotionScore
# ---------------------------------------------------------------------------------------------------------------------------------
def same_summary(a, b):
    return a.keys() == b.keys() and all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a)


@pytest.mark.parametrize("pix", ["yuv420p", "yuv420p10le"])
def test_motion_score_batches(M, Hn, pix):
    """7 frames in batches of 1, 3 and 7 give equal records and summaries, which are the restatement's; with and without a reference"""
    h, w, R = 34, 50, 4
    g = ref.shifted_stream(7, h, w, pix, (1, -2), seed=21)
    d = np.clip(g + np.random.default_rng(22).integers(-9, 10, size=g.shape), 0, ref.top_of(pix))
    gf, df = ref.frames_of(g, pix), ref.frames_of(d, pix)
    cuts = [True, False, False, False, True, False, False]
    for with_ref in (True, False):
        want, want_summary = ref.records(df, gf if with_ref else None, h, w, pix, R=R, cuts=cuts)
        for split in ([7], [3, 3, 1], [1] * 7):
            s, at = M.MotionScore(h, w, fmt_of(Hn, pix), radius=R, device="cuda:0"), 0
            for k in split:
                got = s.update(cuda(df[at:at + k]), cuda(gf[at:at + k]) if with_ref else None, cuts=cuts[at:at + k])
                assert got == want[at:at + k]
                at += k
            assert s.frames == want and same_summary(s.summary(), want_summary)
        assert want[1]["mc_psnr"] is not None and want[4]["mc_psnr"] is None and (want[1]["tc_rmse"] is not None) == with_ref
    s = M.MotionScore(h, w, fmt_of(Hn, pix), radius=R, device="cuda:0")                   # cuts=None: only the first frame is one
    s.update(cuda(df), cuda(gf))
    assert [r["mc_psnr"] is None for r in s.frames] == [True] + [False] * 6


def test_noise_lowers_mc_psnr(M, Hn):
    """every frame the shifted predecessor: tc_rmse 0 and, away from the border, a perfect prediction; the same stream plus independent
    noise of +-2 codes per frame scores a lower mc_psnr and a tc_rmse above 0"""
    pix, h, w = "yuv420p", 70, 130
    g = ref.frames_of(ref.shifted_stream(4, h, w, pix, (2, -3), seed=31), pix)
    noisy = ref.frames_of(ref.shifted_stream(4, h, w, pix, (2, -3), seed=31, noise=2), pix)
    clean_s, noisy_s = (M.MotionScore(h, w, fmt_of(Hn, pix), radius=8, device="cuda:0") for _ in range(2))
    clean_s.update(cuda(g), cuda(g))
    noisy_s.update(cuda(noisy), cuda(g))
    for a, b in zip(clean_s.frames[1:], noisy_s.frames[1:]):
        assert a["tc_rmse"] == 0.0 and a["mc_psnr"] == a["mc_psnr_ref"] == b["mc_psnr_ref"]
        assert b["mc_psnr"] < a["mc_psnr"] and b["tc_rmse"] > 0.0 and a["moving"] == b["moving"] > 0.5
    assert noisy_s.summary()["mc_psnr_global"] < clean_s.summary()["mc_psnr_global"] and clean_s.summary()["tc_rmse_global"] == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# the tool
# ---------------------------------------------------------------------------------------------------------------------------------
def y4m(frames, w, h):
    return b"YUV4MPEG2 W%d H%d F25:1 Ip A1:1 C420p10\n" % (w, h) + b"".join(b"FRAME\n" + f.astype("<u2").tobytes() for f in frames)


def test_tool_with_motion(M, Hn, tmp_path):
    """calculate_video_metrics.py --motion on two 4-frame 10-bit Y4M streams with a scene cut: the new CSV columns are MotionScore's records
    fed VideoScore's cut flags (floats written with repr), each frame line and the `temporal:` line carry the formatted figures; without
    --ref the motion comes from DIST"""
    from fdn_hip import video_metrics as vm
    pix, h, w, R = "yuv420p10le", 34, 38, 5
    a, b = ref.shifted_stream(2, h, w, pix, (1, 2), seed=41), ref.shifted_stream(2, h, w, pix, (0, -1), seed=42) // 8    # a dark second scene
    g = np.concatenate([a, b])
    d = np.clip(g + np.random.default_rng(43).integers(-5, 6, size=g.shape), 0, 1023)
    gf, df = ref.frames_of(g, pix), ref.frames_of(d, pix)
    (tmp_path / "ref.y4m").write_bytes(y4m(gf, w, h))
    (tmp_path / "dist.y4m").write_bytes(y4m(df, w, h))
    fmt = Hn.VideoFormat(pix, "bt601", False, "left")
    tool = [sys.executable, os.path.join(PKG, "calculate_video_metrics.py"), "--batch", "3", "--motion", "--motion-radius", str(R)]
    for with_ref in (True, False):
        vs, ms = vm.VideoScore(h, w, fmt, device="cuda:0"), M.MotionScore(h, w, fmt, radius=R, device="cuda:0")
        recs = vs.update(cuda(df), cuda(gf) if with_ref else None)
        assert [r["cut"] for r in recs] == [True, False, True, False]
        want = ms.update(cuda(df), cuda(gf) if with_ref else None, cuts=[r["cut"] for r in recs])
        assert want == ref.records(df, gf if with_ref else None, h, w, pix, R=R, cuts=[r["cut"] for r in recs])[0]
        out = tmp_path / f"m{int(with_ref)}.csv"
        p = subprocess.run(tool + (["--ref", str(tmp_path / "ref.y4m")] if with_ref else []) + [str(tmp_path / "dist.y4m"), "--csv", str(out)],
                           capture_output=True, timeout=600)
        err = p.stderr.decode()
        print(err)
        assert p.returncode == 0 and "Traceback" not in err and "4 frames scored" in err
        rows = list(csv.reader(open(out)))
        assert rows[0][-5:] == ["mc_psnr", "mc_psnr_ref", "tc_rmse", "moving", "mean_mv"] and len(rows) == 5 and len(rows[0]) == 16
        got = [{k: (None if v == "" else float(v)) for k, v in zip(rows[0][-5:], row[-5:])} for row in rows[1:]]
        assert got == want
        lines = p.stdout.decode().rstrip("\n").split("\n")
        assert len(lines) == 7 and lines[5].startswith("flicker:") and lines[6].startswith("temporal: mc-PSNR ")
        m = want[1]
        if with_ref:
            assert lines[1].endswith(f", mc-PSNR {m['mc_psnr']:.4f} (ref {m['mc_psnr_ref']:.4f}), tc {m['tc_rmse']:.4f}, moving {m['moving']:.3f}")
            assert lines[0].endswith(", mc-PSNR - (ref -), tc -, moving -") and lines[2].endswith(", mc-PSNR - (ref -), tc -, moving -")
            assert f"tc {ms.summary()['tc_rmse']:.4f} " in lines[6]
        else:
            assert lines[1].endswith(f", mc-PSNR {m['mc_psnr']:.4f}, moving {m['moving']:.3f}") and lines[0].endswith(", mc-PSNR -, moving -")
            assert "tc" not in lines[6]
        assert f"mc-PSNR {ms.summary()['mc_psnr']:.4f} dB (over the stream {ms.summary()['mc_psnr_global']:.4f})" in lines[6]
        assert lines[6].endswith(f"search +-{R}")
