"""GPU: exposure fusion (include/fdn_fusion.h, libfdn_fusion.so, fdn_hip.fusion) against the numpy restatement of tests/fusion_ref.py.

  pyr_down, pyr_up, fuse_pyramid   EQUAL to the float32 restatement, bit for bit: the header writes out the order of every fp32 operation
  weights    per value within 32 max(E, 2^-52) of the float64 restatement, E = the restatement's own largest |float64 - longdouble| on
             the case (the rule of tests/test_gpu_sharpness.py for q), held on the float32 handed out: it lies between the float32
             roundings of the interval's ends
  fuse       EQUAL to weights followed by fuse_pyramid; the same bits on a second call and whatever H, W surround the crop, also with the
             second rendering past byte 2^31
  harness    enhance_u8 / validate_u8 with a bracket EQUAL to the composition of the public functions; one driver run in a child process

Shapes: every border case of 1 .. 5 rows and columns; 31, 32 and 33 samples in each axis, and the source sizes whose first level has 31,
32 and 33 (one below, at and above the 32 x 32 tile of the down kernel); several tiles; a crop narrower than its rows."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fusion_ref as ref
from common import fdn_weights
from test_fusion_cpu import check_argument_errors

from common import poison_uninitialized  # noqa: F401  (autouse, tests/common.py: torch.empty is filled with NaN / the integer maximum)
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fdn-tip2025_amd")
T = 32                                                    # FDN_FUSION_TILE (asserted below)
SMALL = [(h, w) for h in range(1, 6) for w in range(1, 6)]
EDGES = [(T - 1, 40), (T, 40), (T + 1, 40), (40, T - 1), (40, T), (40, T + 1), (2 * T - 3, 20), (2 * T, 20), (2 * T + 1, 20), (20, 2 * T - 3),
         (20, 2 * T), (20, 2 * T + 1), (37, 53), (70, 133)]
KS = [1, 2, 3, 7, 16]
EXPONENTS = [(1, 1, 1), (0, 0, 1), (0.5, 2, 1)]


@pytest.fixture(scope="module")
def F():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import fdn_hip
    fdn_hip.lib()   # fail loudly if the HIP extension is not built
    from fdn_hip import fusion
    fusion.lib()
    assert fusion.TILE == T == ref.TILE
    return fusion


def cuda(a):
    return (torch.from_numpy(a) if isinstance(a, np.ndarray) else a).to("cuda:0").contiguous()


def same_bits(got, want):
    """a device tensor and a float32 array hold the same bits (-0.0 and 0.0 differ, a NaN equals itself)"""
    got = got.cpu().numpy()
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (want.shape, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def k_of(i):
    return KS[i % len(KS)]


# ---------------------------------------------------------------------------------------------------------------------------------
# the two resampling steps
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shapes", [SMALL, EDGES], ids=["1..5", "tile edges"])
def test_pyr_down_and_up_bit_exact(F, shapes):
    for n, (h, w) in enumerate(shapes):
        g = np.random.default_rng(1000 * h + w)
        x = (g.random((3, h, w)) * 1.6 - 0.3).astype(np.float32)                     # samples outside [0, 1] too
        same_bits(F.pyr_down(cuda(x)), ref.down(x))
        same_bits(F.pyr_down(cuda(x), clamp=True), ref.down(ref.clamp01(x)))
        big = (g.random((3, h + 3, w + 5)) * 9 - 4).astype(np.float32)               # the crop inside wider rows: the rest is never read
        big[:, :h, :w] = x
        same_bits(F.pyr_down(cuda(big), h, w), ref.down(x))
        c = (g.random((2, (h + 1) // 2, (w + 1) // 2)) * 2 - 0.5).astype(np.float32)
        same_bits(F.pyr_up(cuda(c), h, w), ref.up(c, h, w))


def test_down_of_a_constant_and_up_of_it(F):
    """an exactly representable constant survives both steps at every size, whatever the reflection does"""
    for h, w in SMALL + [(T + 1, 2 * T + 1)]:
        x = torch.full((1, h, w), 0.40625, device="cuda:0")
        d = F.pyr_down(x)
        assert tuple(d.shape) == (1, (h + 1) // 2, (w + 1) // 2) and bool((d == 0.40625).all()) and bool((F.pyr_up(d, h, w) == 0.40625).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# the pyramid on given weights
# ---------------------------------------------------------------------------------------------------------------------------------
def partition_of_unity(K, h, w, seed):
    g = np.random.default_rng(seed)
    p = g.random((K, h, w)) + 1e-3
    return (p / p.sum(axis=0)).astype(np.float32)


def check_pyramid(F, imgs, h, w):
    """imgs [K,3,H,W] float32: fuse_pyramid of [:h, :w] on the device's own weights and on a random partition of unity"""
    K = imgs.shape[0]
    crop = np.ascontiguousarray(imgs[:, :, :h, :w])
    d_imgs = cuda(imgs)
    own = F.weights(d_imgs, h, w)
    assert own.dtype == torch.float32 and tuple(own.shape) == (K, h, w)
    for wts in (own.cpu().numpy(), partition_of_unity(K, h, w, seed=h * 100 + w + K)):
        got = F.fuse_pyramid(d_imgs, cuda(wts), h, w)
        assert tuple(got.shape) == (3, h, w)
        same_bits(got, ref.fuse_pyramid(crop, wts))
    same_bits(F.fuse(d_imgs, h, w), ref.fuse_pyramid(crop, own.cpu().numpy()))        # fuse == weights then fuse_pyramid


def test_fuse_pyramid_bit_exact_on_all_small_shapes(F):
    for n, (h, w) in enumerate(SMALL):
        assert F.dims(h, w) == (ref.levels(h, w), ref.sizes(h, w))
        check_pyramid(F, ref.scene(h, w, k_of(n), seed=n), h, w)


@pytest.mark.parametrize("n", range(len(EDGES)), ids=[f"{h}x{w}" for h, w in EDGES])
def test_fuse_pyramid_bit_exact_at_the_tile_edge_and_on_several_tiles(F, n):
    h, w = EDGES[n]
    check_pyramid(F, ref.scene(h, w, k_of(n), seed=50 + n), h, w)


@pytest.mark.parametrize("K", KS)
def test_fuse_pyramid_bit_exact_for_every_k(F, K):
    check_pyramid(F, ref.scene(37, 53, K, seed=K), 37, 53)


def test_a_crop_narrower_than_its_rows(F):
    """64 x 96 inside H, W = 64, 128: the same bits as from a tight buffer, on a second call, and inside other rows"""
    h, w = 64, 96
    for K in (3, 7):
        g = np.random.default_rng(K)
        imgs = (g.random((K, 3, 64, 128)) * 5 - 2).astype(np.float32)                # what lies outside the crop is far outside [0, 1]
        imgs[:, :, :h, :w] = ref.scene(h, w, K, seed=20 + K)
        check_pyramid(F, imgs, h, w)
        tight = cuda(np.ascontiguousarray(imgs[:, :, :h, :w]))
        first = F.fuse(cuda(imgs), h, w, (0.5, 2, 1))
        assert torch.equal(first, F.fuse(cuda(imgs), h, w, (0.5, 2, 1))) and torch.equal(first, F.fuse(tight, h, w, (0.5, 2, 1)))
        other = torch.full((K, 3, 70, 100), 7.0, device="cuda:0")
        other[:, :, :h, :w] = tight
        assert torch.equal(first, F.fuse(other, h, w, (0.5, 2, 1)))
        assert torch.equal(F.weights(cuda(imgs), h, w), F.weights(tight, h, w))


# ---------------------------------------------------------------------------------------------------------------------------------
# the weights
# ---------------------------------------------------------------------------------------------------------------------------------
def check_weights(F, imgs, exponents, what):
    """imgs [K,3,h,w]: the device's weights within the rule of the restatement; -> the float64 restatement"""
    K, _, h, w = imgs.shape
    got = F.weights(cuda(imgs), h, w, exponents).cpu().numpy()
    q = ref.weights(imgs, exponents)
    E = float(np.abs(q - ref.weights(imgs, exponents, np.longdouble)).max())
    bound = 32 * max(E, 2.0 ** -52)
    lo, hi = (q - bound).astype(np.float32), (q + bound).astype(np.float32)
    worst = float(np.abs(got.astype(np.float64) - q).max())
    print(f"{what} {h}x{w} K={K} exponents {exponents}: E {E:.1e}, bound {bound:.1e}, largest |device - float64| {worst:.1e}")
    assert got.dtype == np.float32 and ((lo <= got) & (got <= hi)).all(), (what, h, w, K, exponents, worst, bound)
    return q, bound, got


@pytest.mark.parametrize("exponents", EXPONENTS, ids=[str(e) for e in EXPONENTS])
def test_weights_within_the_rule(F, exponents):
    for n, (h, w) in enumerate(SMALL + EDGES):
        q, _, got = check_weights(F, ref.scene(h, w, k_of(n), seed=300 + n), exponents, "scene")
        assert abs(float(got.astype(np.float64).sum(axis=0).max()) - 1) <= k_of(n) * 2.0 ** -24 + 1e-12   # K float32 roundings of a partition
    for K in KS:
        check_weights(F, ref.scene(37, 53, K, seed=K), exponents, "every K")


@pytest.mark.parametrize("exponents", EXPONENTS, ids=[str(e) for e in EXPONENTS])
def test_weights_of_flat_gray_renderings(F, exponents):
    """C = S = 0 on a flat gray image: with the contrast or the saturation in the product the 1e-12 term decides, and every weight is 1 / K"""
    for K in KS:
        levels = np.linspace(0.1, 0.9, K) if K > 1 else np.array([0.5])
        imgs = np.broadcast_to(levels.astype(np.float32)[:, None, None, None], (K, 3, 9, 11)).copy()
        q, bound, got = check_weights(F, imgs, exponents, "flat gray")
        if exponents[0] or exponents[1]:
            lo, hi = np.float32(1.0 / K - bound), np.float32(1.0 / K + bound)
            assert ((lo <= got) & (got <= hi)).all(), (K, exponents, got.min(), got.max())
        else:
            assert K <= 2 or got[K // 2].min() > got[0].max()                          # well-exposedness alone prefers the middle gray


# ---------------------------------------------------------------------------------------------------------------------------------
# offsets, errors
# ---------------------------------------------------------------------------------------------------------------------------------
def test_second_rendering_past_byte_2_31(F):
    """K = 2, 37 x 37 inside H = W = 16384: 3 * 2^28 floats per rendering, so the second starts at byte 3 * 2^30; only the crops are written"""
    h = w = 37
    imgs = ref.scene(h, w, 2, seed=77)
    tight = cuda(imgs)
    want_w, want = F.weights(tight, h, w), F.fuse(tight, h, w)
    big = torch.empty((2, 3, 16384, 16384), dtype=torch.float32, device="cuda:0")
    assert big[1].data_ptr() - big.data_ptr() == 3 * 2 ** 30 > 2 ** 31
    big[:, :, :h, :w] = tight
    assert torch.equal(F.weights(big, h, w), want_w) and torch.equal(F.fuse(big, h, w), want)
    same_bits(want, ref.fuse_pyramid(imgs, want_w.cpu().numpy()))
    del big
    torch.cuda.empty_cache()


def test_argument_errors_on_the_device(F):
    """with a device present every refusal still comes before any launch: the pointers of check_argument_errors are never dereferenced"""
    check_argument_errors(F.lib())
    torch.cuda.synchronize()
    from fdn_hip import FdnHipError
    z = torch.zeros((3, 3, 8, 8), device="cuda:0")
    with pytest.raises(FdnHipError, match="weights must be fp32"):
        F.fuse_pyramid(z, torch.zeros((2, 8, 8), device="cuda:0"), 8, 8)
    with pytest.raises(FdnHipError, match="must be float32"):
        F.weights(z.double(), 8, 8)
    with pytest.raises(FdnHipError, match="must be contiguous"):
        F.weights(z[:, :, :, ::2], 8, 4)


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end on the tamed weights
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net(F):
    from basicsr.models.archs.FDN_arch import FDN
    m = FDN()
    m.load_state_dict(fdn_weights(tame=0.03), strict=True)
    return m.to("cuda:0").eval()


def frame(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


BRACKET = (-1, 0, 1)


def test_enhance_u8_with_a_bracket_is_the_composition(F, net):
    from fdn_hip import harness
    img = cuda(frame(50, 60, seed=5))
    ratio = torch.tensor([[0.3]], device="cuda:0")
    got = harness.enhance_u8(net, None, img, bgr=False, ratio_mode="fixed", ratio=ratio, bracket=BRACKET)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1, 50, 60, 3)
    with torch.no_grad():
        x, h, w = harness.preprocess(img, bgr=False)
        rs = F.bracket_ratios(ratio, BRACKET)[0]
        assert rs.flatten().tolist() == [np.float32(0.3) * 2, np.float32(0.3), np.float32(0.3) / 2]
        res = net(x.expand(3, -1, -1, -1).contiguous(), ratio_i=rs.contiguous(), device=x.device)[0].contiguous()
        assert tuple(res.shape) == (3, 3, 64, 64)
        want = harness.postprocess(F.fuse(res, h, w).unsqueeze(0), h, w, bgr=False)
    assert torch.equal(got, want)
    plain = harness.enhance_u8(net, None, img, bgr=False, ratio_mode="fixed", ratio=ratio)
    assert not torch.equal(got, plain)                                                 # the bracket does something
    # other exponents reach the weights; one stop per forward is the same frame
    got2 = harness.enhance_u8(net, None, img, bgr=False, ratio_mode="fixed", ratio=ratio, bracket=BRACKET, fusion=(0, 0, 1), batch=1)
    with torch.no_grad():
        one = torch.cat([net(x, ratio_i=rs[k:k + 1].contiguous(), device=x.device)[0] for k in range(3)]).contiguous()
        assert torch.equal(got2, harness.postprocess(F.fuse(one, h, w, (0, 0, 1)).unsqueeze(0), h, w, bgr=False))
    # a bracket of the one stop 0: the frame itself, through a pyramid and back
    single = harness.enhance_u8(net, None, img, bgr=False, ratio_mode="fixed", ratio=ratio, bracket=(0,))
    diff = int((single.int() - plain.int()).abs().max())
    print(f"bracket (0,) against no bracket: largest difference {diff} code(s)")
    assert diff <= 1


def test_enhance_u8_tiled_with_a_bracket_is_the_composition(F, net):
    from fdn_hip import harness, tiling
    img = cuda(frame(50, 60, seed=6))
    ratio = torch.tensor([[0.25]], device="cuda:0")
    got = harness.enhance_u8(net, None, img, bgr=False, ratio_mode="fixed", ratio=ratio, bracket=BRACKET, tile=(32, 32), overlap=8,
                             blend="feather")
    with torch.no_grad():
        tiles, ij = tiling.split_u8(img, 32, 32, bgr=False, overlap=8)
        n = tiles.shape[0]
        assert n > 1
        merged = [tiling.merge(tiling.run_tiles(net, tiles, r.expand(n, 1).contiguous(), 8), ij, 50, 60, "feather")
                  for r in F.bracket_ratios(ratio, BRACKET)[0]]
        want = harness.postprocess(F.fuse(torch.cat(merged), 50, 60).unsqueeze(0), 50, 60, bgr=False)
    assert torch.equal(got, want)
    out, r = harness.enhance_frame_tiled(net, None, img, (32, 32), bgr=False, ratio_mode="fixed", ratio=ratio, overlap=8, blend="feather",
                                         bracket=BRACKET, run=lambda t, rr: tiling.run_tiles(net, t, rr, 4))     # a caller's run serves every stop
    assert torch.equal(out, want[0]) and torch.equal(r, ratio.expand(n, 1))


def test_validate_u8_with_a_bracket_scores_that_frame(F, net):
    from fdn_hip import harness
    from fdn_hip.metrics import calculate_psnr_ssim_u8
    lq, gt = cuda(frame(50, 60, seed=7)[None] // 4), cuda(frame(50, 60, seed=7)[None])
    plain = harness.validate_u8(net, None, lq, gt, ratio_mode="gt", bgr=False)
    out, psnr, ssim, ratio = harness.validate_u8(net, None, lq, gt, ratio_mode="gt", bgr=False, bracket=BRACKET, fusion=(1, 0.5, 1))
    assert torch.equal(ratio, plain[3])                                                # the ratio without the stops
    want = harness.enhance_u8(net, None, lq, bgr=False, ratio_mode="fixed", ratio=ratio, bracket=BRACKET, fusion=(1, 0.5, 1))
    assert torch.equal(out, want) and not torch.equal(out, plain[0])
    assert (psnr, ssim) == tuple(calculate_psnr_ssim_u8(out, gt, crop_border=0, bgr=False))
    fixed = harness.validate_u8(net, None, lq, gt, ratio_mode="fixed", ratio=ratio, bgr=False)     # a caller's ratio: the same frame as gt's
    assert torch.equal(fixed[0], plain[0]) and fixed[1:3] == plain[1:3]


def test_a_driver_run_with_a_bracket(F, net, tmp_path):
    """inference_fdn_lolblur.py --ratio 0.3 --bracket -1,0,1 in a fresh child process writes the frame enhance_u8 returns"""
    from PIL import Image
    from fdn_hip import harness
    img = frame(50, 60, seed=8)
    (tmp_path / "in").mkdir()
    Image.fromarray(img).save(tmp_path / "in" / "a.png")
    torch.save({"params": fdn_weights(tame=0.03)}, tmp_path / "fdn.pth")
    run = subprocess.run([sys.executable, os.path.join(PKG, "inference_fdn_lolblur.py"), "--fdn", str(tmp_path / "fdn.pth"), "--ratio", "0.3",
                          "--bracket", "-1,0,1", "--fusion-weights", "1,1,0.5", "--input", str(tmp_path / "in" / "*.png"), "--output",
                          str(tmp_path / "out")], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0, run.stderr
    want = harness.enhance_u8(net, None, cuda(img), bgr=False, ratio_mode="fixed", ratio=torch.tensor([[0.3]], device="cuda:0"),
                              bracket=BRACKET, fusion=(1, 1, 0.5))
    assert np.array_equal(np.array(Image.open(tmp_path / "out" / "a.png")), want[0].cpu().numpy())
