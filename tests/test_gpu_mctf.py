"""GPU: motion-compensated temporal denoising (include/fdn_mctf.h, libfdn_mctf.so, fdn_hip.mctf) against the float32 numpy restatement of
tests/mctf_ref.py.  Every operation of the definition is ordered and rounded once, so every comparison is for bit equality (the int32
views); out and kmap come from torch.empty under the poison fixture, so a pixel the kernel does not write is a NaN.

Shapes h x w (H x W), B - the smallest at which a halo-tiled, block-indexed kernel can go wrong (the kernel's tile is 16 rows x 64 columns):
    1 x 1, 2 x 2,      B 2    every neighbour is a clamp, one partial block
    16 x 16,           B 2    one full block
    18 x 34 (32 x 64), B 3    2 x 3 blocks with partial last ones; the padding holds NaN and must never be read
    34 x 50 (64 x 64), B 3    odd dense strides against padded input strides; three tile rows; NaN among cur's own pixels
    70 x 130,          B 3    5 x 9 blocks, 5 x 3 tiles; vectors of +-16 leave the frame on every side
    17 x 65,           B 2    one pixel taller and one pixel wider than a tile
    16 x 128,          B 2    exactly two tiles wide
Data: cur uniform in [-0.2, 1.2] so that the clamp acts; a random prev and prev = None; vectors of +-16 and below, arbitrary shorts with
-32768 and 32767 among them, and vectors from a real search; identical frames; a ramp that takes D across the threshold; stats word 0 at
cut_limit and one above; kmap wanted and not wanted.  Then the layers above: TemporalDenoiser.step across batch boundaries,
enhance_yuv420(denoise=) on the untiled and the tiled route, and inference_fdn_video.py --temporal-denoise through pipes."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mctf_ref as ref
import temporal_ref
from common import fdn_weights, lpnet_weights
from test_mctf_cpu import check_argument_errors

from common import poison_uninitialized  # noqa: F401  (autouse, tests/common.py: torch.empty is filled with NaN / the integer maximum)
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fdn-tip2025_amd")
F = np.float32
BIG = 2 ** 62                                                        # in the words of stats that must not be read
THRESHOLD = 0.65                                                     # of the random cases: independent uniform frames differ by about that


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import fdn_hip
    fdn_hip.lib()   # fail loudly if the HIP extension is not built
    from fdn_hip import mctf
    mctf.lib()
    return mctf


@pytest.fixture(scope="module")
def Hn(M):
    from fdn_hip import harness
    return harness


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0").contiguous()


def same_bits(a, b):
    return np.array_equal(ref.bits(a), ref.bits(b))


def stats_of(word0):
    return np.array([[v, BIG, -BIG, BIG] for v in word0], dtype=np.int64)


def run(M, cur, prev, mv, stats, h, w, strength, threshold, limit):
    """mctf.blend with the weights wanted and not wanted -> host (out, k); the two outs must be the same bits"""
    t_cur, t_prev = cuda(cur), (None if prev is None else cuda(prev))
    t_mv, t_stats = cuda(np.asarray(mv).astype(np.int16)), cuda(np.asarray(stats, dtype=np.int64))
    out, k = M.blend(t_cur, t_prev, t_mv, t_stats, h, w, strength, threshold, limit, kmap=True)
    alone = M.blend(t_cur, t_prev, t_mv, t_stats, h, w, strength, threshold, limit)
    assert out.shape == (cur.shape[0], 3, h, w) and k.shape == (cur.shape[0], h, w) and out.dtype == k.dtype == torch.float32
    assert torch.equal(out.view(torch.int32), alone.view(torch.int32))
    return out.cpu().numpy(), k.cpu().numpy()


def vectors(kind, g, B, h, w):
    nby, nbx = ref.block_grid(h, w)
    if kind == "near":                                               # up to +-16, the ends of the range among them
        mv = g.integers(-16, 17, size=(B, nby, nbx, 2))
        mv.reshape(-1)[::3] = g.choice([-16, 16], size=mv.reshape(-1)[::3].shape)
    else:                                                            # any short
        mv = g.integers(-32768, 32768, size=(B, nby, nbx, 2))
        mv.reshape(-1)[:4] = [-32768, 32767, 32767, -32768]
    return mv


@functools.lru_cache(maxsize=None)
def random_case(shape, kind):
    """host data of one shape and its restated answers with and without a frame before, computed once"""
    h, w, H, W, B = shape
    g = np.random.default_rng(1000 * h + 10 * w + len(kind))
    cur = np.full((B, 3, H, W), np.nan, dtype=F)                     # what lies outside h x w must never be read
    cur[:, :, :h, :w] = g.uniform(-0.2, 1.2, size=(B, 3, h, w))
    if (h, w) == (34, 50):
        cur[:, :, 5, 7] = np.nan                                     # a NaN of cur's own becomes 0
        cur[1, 2, 33, 49] = np.nan
    prev = g.uniform(0.0, 1.0, size=(3, h, w)).astype(F)
    mv = vectors(kind, g, B, h, w)
    stats = stats_of([0] * B)
    inv = ref.inv_of(THRESHOLD)
    with_prev = ref.blend(cur, prev, mv, stats, h, w, 0.6, inv, 10)
    without = ref.blend(cur, None, mv, stats, h, w, 0.6, inv, 10)
    for a in with_prev + without:
        a.setflags(write=False)
    return cur, prev, mv, stats, with_prev, without


@pytest.mark.parametrize("kind", ["near", "any"])
@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: "%dx%d-%dx%d-B%d" % s)
def test_random_frames_equal_restatement(M, shape, kind):
    h, w, H, W, B = shape
    cur, prev, mv, stats, (want, want_k), (want0, want_k0) = random_case(shape, kind)
    assert not np.isnan(want).any() and not np.isnan(want0).any()
    if h * w >= 256:
        assert want0[0].min() == 0.0 and want0[0].max() == 1.0                            # the clamp acts on both sides
        assert (want_k == 0).any() and (want_k > 0).any() and (want_k[1:] > 0).any()      # both sides of the threshold, in later frames too
    if kind == "any":
        assert mv.min() == -32768 and mv.max() == 32767
    out, k = run(M, cur, prev, mv, stats, h, w, 0.6, THRESHOLD, 10)
    assert same_bits(k, want_k) and same_bits(out, want)
    # no frame before: frame 0 is clamp01(cur) with k = 0, the others are filtered against it
    out, k = run(M, cur, None, mv, stats, h, w, 0.6, THRESHOLD, 10)
    assert same_bits(k, want_k0) and same_bits(out, want0)
    assert not k[0].any() and same_bits(out[0], ref.clamp01(cur[0, :, :h, :w]))


def test_vectors_from_a_real_search(M, Hn):
    """a noisy moving texture, posted to 4:2:0 samples and searched as TemporalDenoiser does it; the defaults"""
    from fdn_hip import motion
    fmt = Hn.VideoFormat("yuv420p", "bt709", False, "left")
    for (h, w, H, W, B), step in (((18, 34, 32, 64, 3), (1, -1)), ((34, 50, 64, 64, 3), (2, -3)), ((70, 130, 70, 130, 3), (-3, 5))):
        _, noisy = ref.noisy_stream(B + 1, h, w, step, 0.03, seed=h)
        cur = np.full((B, 3, H, W), np.nan, dtype=F)
        cur[:, :, :h, :w] = noisy[1:]
        guide = Hn.postprocess_yuv420(cuda(noisy), h, w, fmt)
        mv, _, stats = motion.search(guide[1:], guide[:1], h, w, fmt, radius=8)
        limit = M.cut_limit(0.10, h, w, 8)
        out, k = M.blend(cuda(cur), cuda(noisy[0]), mv, stats, h, w, 0.6, 0.12, limit, kmap=True)
        mv_h, stats_h = mv.cpu().numpy(), stats.cpu().numpy()
        assert mv_h.any() and 0 < stats_h[:, 0].min() and stats_h[:, 0].max() <= limit
        want, want_k = ref.blend(cur, noisy[0], mv_h, stats_h, h, w, 0.6, ref.inv_of(0.12), limit)
        assert same_bits(k.cpu().numpy(), want_k) and same_bits(out.cpu().numpy(), want)
        assert want_k.mean() > 0.3                                                      # the prediction fits: the filter is at work


def test_identical_frames(M):
    h, w = 34, 50
    g = np.random.default_rng(12)
    one = g.uniform(0.0, 1.0, size=(3, h, w)).astype(F)
    cur = np.repeat(one[None], 3, axis=0)
    mv = np.zeros((3, 3, 4, 2), dtype=np.int64)
    out, k = run(M, cur, one, mv, stats_of([0] * 3), h, w, 0.6, 0.12, 0)
    want, want_k = ref.blend(cur, one, mv, stats_of([0] * 3), h, w, 0.6, ref.inv_of(0.12), 0)
    assert same_bits(k, want_k) and same_bits(out, want) and np.all(k == F(0.6))
    assert np.abs(out.astype(np.float64) - cur).max() < 1e-6


def test_threshold_edge(M):
    """cur = prev + a ramp along x from 0.10 to 0.15, zero vectors, threshold 0.125: D follows the ramp, so some pixels lie just below the
    threshold and some just above; k is 0 exactly where D >= threshold and those pixels come back unchanged"""
    h, w = 20, 200
    g = np.random.default_rng(13)
    prev = g.uniform(0.0, 0.5, size=(3, h, w)).astype(F)
    cur = (prev + np.linspace(0.10, 0.15, w, dtype=F)[None, None, :])[None]
    mv = np.zeros((1, 2, 13, 2), dtype=np.int64)
    _, want_k, D, _ = ref.blend_frame(ref.clamp01(cur[0]), prev, mv[0], 0.6, ref.inv_of(0.125))
    assert ((D > 0.1245) & (D < 0.125)).any() and ((D >= 0.125) & (D < 0.1255)).any()
    out, k = run(M, cur, prev, mv, stats_of([0]), h, w, 0.6, 0.125, 0)
    want, want_k2 = ref.blend(cur, prev, mv, stats_of([0]), h, w, 0.6, ref.inv_of(0.125), 0)
    assert same_bits(want_k, want_k2[0]) and same_bits(k, want_k2) and same_bits(out, want)
    hot = D >= F(0.125)
    assert not k[0][hot].any() and k[0][~hot].all() and same_bits(out[0][:, hot], cur[0][:, hot])


def test_scene_cut_is_decided_on_the_device(M):
    """stats word 0 at cut_limit: filtered; one above: returned clamped with k = 0, and the next frame is filtered against that"""
    shape = (34, 50, 64, 64, 3)
    h, w, H, W, B = shape
    cur, prev, mv, _, _, _ = random_case(shape, "near")
    limit = 43350
    stats = stats_of([limit, limit + 1, limit])
    want, want_k = ref.blend(cur, prev, mv, stats, h, w, 0.6, ref.inv_of(THRESHOLD), limit)
    out, k = run(M, cur, prev, mv, stats, h, w, 0.6, THRESHOLD, limit)
    assert same_bits(k, want_k) and same_bits(out, want)
    assert k[0].any() and not k[1].any() and k[2].any() and same_bits(out[1], ref.clamp01(cur[1, :, :h, :w]))
    out, k = run(M, cur, prev, mv, stats_of([limit + 1] * 3), h, w, 0.6, THRESHOLD, limit)
    assert not k.any() and same_bits(out, ref.clamp01(cur[:, :, :h, :w]))
    out, k = run(M, cur, prev, mv, stats_of([2 ** 40] * 3), h, w, 0.6, THRESHOLD, 2 ** 40)    # the comparison is in 64 bits
    assert k[0].any() and k[2].any()


def test_strength_zero_and_one(M):
    shape = (18, 34, 32, 64, 3)
    h, w, H, W, B = shape
    cur, prev, mv, stats, _, _ = random_case(shape, "near")
    out, k = run(M, cur, prev, mv, stats, h, w, 0.0, THRESHOLD, 10)
    assert not k.any() and same_bits(out, ref.clamp01(cur[:, :, :h, :w]))
    out, k = run(M, cur, prev, mv, stats, h, w, 1.0, THRESHOLD, 10)
    want, want_k = ref.blend(cur, prev, mv, stats, h, w, 1.0, ref.inv_of(THRESHOLD), 10)
    assert same_bits(k, want_k) and same_bits(out, want)


def test_argument_errors_with_a_device(M):
    check_argument_errors(M.lib())


# ---------------------------------------------------------------------------------------------------------------------------------
# TemporalDenoiser
# ---------------------------------------------------------------------------------------------------------------------------------
def test_step_carries_the_stream_across_batches(M, Hn):
    """four frames at once = four calls of one frame, bit for bit, and both are the restatement fed the device's own vectors; after
    reset() the next frame is a first frame"""
    from fdn_hip import motion
    h, w, H, W = 34, 50, 64, 64
    fmt = Hn.VideoFormat("yuv420p10le", "bt709", False, "left")
    _, noisy = ref.noisy_stream(4, h, w, (2, -3), 0.03, seed=21)
    res = np.full((4, 3, H, W), np.nan, dtype=F)
    res[:, :, :h, :w] = noisy * F(1.3) - F(0.1)                                       # beyond [0, 1] here and there
    t_res = cuda(res)
    whole = M.TemporalDenoiser(h, w, fmt, device="cuda:0")
    out = whole.step(t_res)
    assert out.shape == (4, 3, h, w) and out.dtype == torch.float32
    single = M.TemporalDenoiser(h, w, fmt, device="cuda:0")
    one = torch.cat([single.step(t_res[t:t + 1]) for t in range(4)])
    assert torch.equal(one.view(torch.int32), out.view(torch.int32))
    split = M.TemporalDenoiser(h, w, fmt, device="cuda:0")
    two = torch.cat([split.step(t_res[:3]), split.step(t_res[3:])])
    assert torch.equal(two.view(torch.int32), out.view(torch.int32))
    guide = Hn.postprocess_yuv420(t_res, h, w, fmt)
    mv, _, stats = motion.search(guide, None, h, w, fmt, radius=8)
    assert whole.cut_limit == M.cut_limit(0.10, h, w, 10) == 173910
    want, want_k = ref.blend(res, None, mv.cpu().numpy(), stats.cpu().numpy(), h, w, 0.6, ref.inv_of(0.12), whole.cut_limit)
    assert same_bits(out.cpu().numpy(), want) and not want_k[0].any() and all(want_k[t].mean() > 0.2 for t in (1, 2, 3))
    assert same_bits(want[0], ref.clamp01(res[0, :, :h, :w])) and not same_bits(want[1], ref.clamp01(res[1, :, :h, :w]))
    # a further frame is filtered; after reset() the same frame comes back clamped
    more = whole.step(t_res[1:2])
    assert not torch.equal(more, t_res[1:2, :, :h, :w].clamp(0, 1))
    whole.reset()
    first = whole.step(t_res[1:2])
    assert same_bits(first.cpu().numpy(), ref.clamp01(res[1:2, :, :h, :w]))
    with pytest.raises(Hn.FdnHipError, match="cannot crop"):
        whole.step(t_res[:, :, :20].contiguous())


# ---------------------------------------------------------------------------------------------------------------------------------
# enhance_yuv420(denoise=...)
# ---------------------------------------------------------------------------------------------------------------------------------
def load(mod, sd):
    mod.load_state_dict(sd, strict=True)
    return mod.to("cuda:0").eval()


@pytest.fixture(scope="module")
def nets(Hn):
    from basicsr.models.archs.FDN_arch import FDN
    from basicsr.models.archs.LPNet_arch import I_predict_net
    return load(FDN(), fdn_weights(tame=0.03)), load(I_predict_net(), lpnet_weights())


def test_enhance_untiled_with_denoiser(M, Hn, nets):
    """enhance_yuv420(denoise=d) = postprocess_yuv420(d2.step(the forward's result)), byte for byte, over two calls that continue one stream;
    without a denoiser the output is what it was"""
    net, lp = nets
    h, w = 34, 38
    fmt = Hn.VideoFormat("yuv420p", "bt601", False, "left")
    frames = cuda(temporal_ref.scene_frames())
    d, d2 = M.TemporalDenoiser(h, w, fmt, device="cuda:0"), M.TemporalDenoiser(h, w, fmt, device="cuda:0")
    for part in (frames[:3], frames[3:]):
        got = Hn.enhance_yuv420(net, lp, part, h, w, fmt, denoise=d)
        plain = Hn.enhance_yuv420(net, lp, part, h, w, fmt)
        with torch.no_grad():
            forward = Hn._forward(net, lp, Hn.preprocess_yuv420(part, h, w, fmt)[0], "lolblur", None).contiguous()
            assert torch.equal(plain, Hn.postprocess_yuv420(forward, h, w, fmt))
            want = Hn.postprocess_yuv420(d2.step(forward), h, w, fmt)
        assert got.shape == part.shape and got.dtype == torch.uint8 and torch.equal(got, want)
        print("samples the denoiser changed:", int((got != plain).sum()), "of", got.numel())
    with pytest.raises(ValueError, match="temporal denoiser is for 34x38 8-bit frames"):
        Hn.enhance_yuv420(net, lp, frames, h, w, Hn.VideoFormat("yuv420p10le"), denoise=d)


def test_enhance_tiled_with_denoiser(M, Hn, nets):
    """two 70 x 90 frames, tile (32, 64), a fixed ratio: the merged fp32 frame goes through the denoiser before it is posted"""
    from fdn_hip import tiling
    net, lp = nets
    h, w = 70, 90
    fmt = Hn.VideoFormat("yuv420p", "bt709", False, "left")
    frames = cuda(temporal_ref.scene_frames(seed=9, h=h, w=w)[:2])
    ratio = torch.tensor([[0.31], [0.29]], device="cuda:0")
    kw = dict(ratio_mode="fixed", ratio=ratio, tile=(32, 64), ratio_from="frame", batch=4)
    d, d2 = M.TemporalDenoiser(h, w, fmt, device="cuda:0"), M.TemporalDenoiser(h, w, fmt, device="cuda:0")
    got = Hn.enhance_yuv420(net, None, frames, h, w, fmt, denoise=d, **kw)
    plain = Hn.enhance_yuv420(net, None, frames, h, w, fmt, **kw)
    ch, cw = tiling.effective_crop(h, w, 32, 64)
    merged = [tiling.forward_tiled(net, None, Hn.preprocess_yuv420(frames[b:b + 1], h, w, fmt, pad=False)[0], ch, cw, batch=4, ratio=ratio[b:b + 1])
              for b in range(2)]
    assert merged[0].shape == (1, 3, h, w)
    assert torch.equal(plain, torch.cat([Hn.postprocess_yuv420(m, h, w, fmt) for m in merged]))
    want = torch.cat([Hn.postprocess_yuv420(d2.step(m), h, w, fmt) for m in merged])
    assert got.shape == frames.shape and torch.equal(got, want)
    print("samples the denoiser changed:", int((got != plain).sum()), "of", got.numel())


def test_driver_temporal_denoise(M, Hn, nets, tmp_path):
    """the four scene frames as Y4M through pipes with --temporal-denoise and its three companions, in batches of 3: the harness's bytes"""
    net, lp = nets
    torch.save({"params": fdn_weights(tame=0.03)}, tmp_path / "fdn.pth")
    torch.save({"params": lpnet_weights()}, tmp_path / "lpnet.pth")
    frames = temporal_ref.scene_frames()
    header = b"YUV4MPEG2 W38 H34 F25:1 Ip A1:1 C420mpeg2\n"
    stream = header + b"".join(b"FRAME\n" + f.tobytes() for f in frames)
    run = subprocess.run([sys.executable, os.path.join(PKG, "inference_fdn_video.py"), "--fdn", str(tmp_path / "fdn.pth"), "--lpnet",
                          str(tmp_path / "lpnet.pth"), "--batch", "3", "--temporal-denoise", "0.8", "--denoise-threshold", "0.2",
                          "--denoise-radius", "4", "--denoise-cut", "0.5", "-", "-"], input=stream, capture_output=True, timeout=600)
    err = run.stderr.decode()
    print(err)
    assert run.returncode == 0, err
    assert err.rstrip("\n").split("\n")[-1] == "4 frames -> -"
    fmt = Hn.VideoFormat("yuv420p", "bt601", False, "left")
    d = M.TemporalDenoiser(34, 38, fmt, 0.8, 0.2, 4, 0.5, device="cuda:0")
    dev = cuda(frames)
    want = torch.cat([Hn.enhance_yuv420(net, lp, part, 34, 38, fmt, denoise=d) for part in (dev[:3], dev[3:])]).cpu().numpy()
    assert run.stdout == header + b"".join(b"FRAME\n" + fr.tobytes() for fr in want)
