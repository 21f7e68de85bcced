"""GPU: the geometric self-ensemble - the four entry points of include/fdn_ensemble.h, fdn_hip.ensemble, and the `ensemble` keyword of
fdn_hip.harness.enhance_u8 / validate_u8 / enhance_frame_tiled and fdn_hip.tiling.run_tiles.

The kernels move values, divide uint8 by 255 and form one ordered fp32 sum with one division, so everything is held by equality: the
copies against fdn_pre_u8 of the torch-transformed image (tests/d4_ref.py) and against the torch transform plus reflect padding; the mean
against the restatement's ordered sum on the CPU; the uint8 form against fdn_d4_mean + fdn_post_u8; and enhance_u8(ensemble=e) against the
composition of single eager passes on torch-transformed frames, all fed the ratio of the untransformed frame.  Kernel shapes (h, w), B = 2:

    33 x 65    odd, padded in both axes to 64 x 96 and, transposed, to 96 x 64
    70 x 90    two staging tiles along either axis, the second one across the image's edge and its padding
    32 x 32    no padding, one tile
    34 x 300   crosses a 256-wide block
    5 x 7      smaller than any staging tile; padding to 32 would need pad >= size, so H, W = h', w'

Every output buffer is filled with NaN (fp32) or 0xFF and then 0x00 (uint8) before the call, so a pixel that is not written shows.
"""
import ctypes

import numpy as np
import pytest
import torch

import d4_ref as ref
import fdn_oracle as O
from common import fdn_weights, lpnet_weights

from common import poison_uninitialized  # noqa: F401  (autouse, tests/common.py: torch.empty is filled with NaN / the integer maximum)
pytestmark = pytest.mark.gpu

SHAPES = [(33, 65), (70, 90), (32, 32), (34, 300), (5, 7)]
IDS = [f"{h}x{w}" for h, w in SHAPES]
B = 2


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import fdn_hip
    fdn_hip.lib()   # fail loudly if the HIP extension is not built
    from fdn_hip import ensemble
    return ensemble


def cuda(a):
    return (torch.from_numpy(a) if isinstance(a, np.ndarray) else a).to("cuda:0").contiguous()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def padded(h, w):
    """the padded size the kernel tests use: the x32 grid, or the size itself where that would need pad >= size"""
    from fdn_hip.harness import padded_size
    H, W = padded_size(h, w)
    return (H, W) if H - h < h and W - w < w else (h, w)


def images(h, w):
    g = torch.Generator().manual_seed(1000 * h + w)
    return torch.randint(0, 256, (B, h, w, 3), generator=g, dtype=torch.uint8)


def to_u8(res, bgr):
    """tensor2img on the CPU: fp32 [B,3,h,w] -> clamp(0,1) * 255, round half to even -> uint8 [B,h,w,3]"""
    v = (res.clamp(0, 1) * 255.0).round().to(torch.uint8).permute(0, 2, 3, 1)
    return (v.flip(-1) if bgr else v).contiguous()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_pre_u8_equals_pre_u8_of_the_transformed_image(E, shape):
    import fdn_hip
    lib, st = fdn_hip.lib(), fdn_hip.stream
    h, w = shape
    img = images(h, w)
    dimg = cuda(img)
    for bgr in (1, 0):
        single = {}
        for k in range(8):
            hp, wp = ref.d4_shape(k, h, w)
            H, W = padded(hp, wp)
            t = cuda(ref.transform(img, k, (1, 2)))
            want = torch.full((B, 3, H, W), float("nan"), device="cuda:0")
            fdn_hip.check(lib.fdn_pre_u8(ptr(t), ptr(want), B, hp, wp, H, W, bgr, st()), "fdn_pre_u8")
            got = torch.full((1, B, 3, H, W), float("nan"), device="cuda:0")
            fdn_hip.check(lib.fdn_d4_pre_u8(ptr(dimg), ptr(got), B, h, w, H, W, 1 << k, bgr, st()), "fdn_d4_pre_u8")
            assert not torch.isnan(want).any()
            assert torch.equal(got[0], want), f"code {k}, swap_rb={bgr}"
            single[k] = want
            if (H, W) != (hp, wp):                                   # the wrapper pads to the same grid
                out, ghp, gwp = E.pre_u8(dimg, 1 << k, bgr=bool(bgr))
                assert (ghp, gwp) == (hp, wp) and torch.equal(out[0], want)
        for mask in (0x0F, 0xF0):
            ks = ref.codes(mask)
            H, W = single[ks[0]].shape[-2:]
            got = torch.full((4, B, 3, H, W), float("nan"), device="cuda:0")
            fdn_hip.check(lib.fdn_d4_pre_u8(ptr(dimg), ptr(got), B, h, w, H, W, mask, bgr, st()), "fdn_d4_pre_u8")
            assert torch.equal(got, torch.stack([single[k] for k in ks])), f"mask {mask:#x}, swap_rb={bgr}"


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_apply_equals_the_torch_transform_and_padding(E, shape):
    import fdn_hip
    lib, st = fdn_hip.lib(), fdn_hip.stream
    h, w = shape
    g = torch.Generator().manual_seed(7 * h + w)
    x = torch.rand(B, 3, h, w, generator=g) * 3.0 - 1.0                # values outside [0, 1] too: nothing is computed
    assert x.min() < -0.5 and x.max() > 1.5
    dx = cuda(x)
    for mask in (0x0F, 0xF0, 0x01, 0x20, 0x0A, 0xD0):
        ks = ref.codes(mask)
        hp, wp = ref.d4_shape(ks[0], h, w)
        H, W = padded(hp, wp)
        want = torch.stack([ref.reflect_pad(ref.transform(x, k, (-2, -1)), H, W) for k in ks])
        got = torch.full((len(ks), B, 3, H, W), float("nan"), device="cuda:0")
        fdn_hip.check(lib.fdn_d4_apply(ptr(dx), ptr(got), B, h, w, H, W, mask, st()), "fdn_d4_apply")
        assert torch.equal(got.cpu(), want), f"mask {mask:#x}"
    out, hp, wp = E.apply(dx, 0xF0, pad=False)
    assert (hp, wp) == (w, h) and out.shape == (4, B, 3, w, h)
    assert torch.equal(out.cpu(), torch.stack([ref.transform(x, k, (-2, -1)) for k in range(4, 8)]))


def results_with_ties(h, w, mask, seed):
    """{k: fp32 [B,3,H_k,W_k]} for the codes of mask: values in [-0.2, 1.2], and over a third of the pixels every copy holds the same
    (j + 0.5) / 255 where it maps back to, so that the mean lands on the half-to-even tie of the uint8 rounding"""
    g = torch.Generator().manual_seed(seed)
    planted = (torch.rand(B, 1, h, w, generator=g) < 0.35).expand(B, 3, h, w)
    ties = (torch.randint(0, 255, (B, 3, h, w), generator=g).float() + 0.5) / 255.0
    res = {}
    for k in ref.codes(mask):
        hp, wp = ref.d4_shape(k, h, w)
        H, W = padded(hp, wp)
        r = torch.rand(B, 3, H, W, generator=g) * 1.4 - 0.2
        m, t = ref.transform(planted, k, (-2, -1)), ref.transform(ties, k, (-2, -1))
        r[..., :hp, :wp][m] = t[m]
        res[k] = r
    return res


def halves(res, mask):
    """the results as the entry points take them: (res_a [Ka,...] or None, res_b [Kb,...] or None) on the device"""
    a = [res[k] for k in ref.codes(mask) if not k & 4]
    b = [res[k] for k in ref.codes(mask) if k & 4]
    return (cuda(torch.stack(a)) if a else None), (cuda(torch.stack(b)) if b else None)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_mean_and_post_u8_equal_the_ordered_sum(E, shape):
    import fdn_hip
    from fdn_hip import harness
    lib, st = fdn_hip.lib(), fdn_hip.stream
    h, w = shape
    ties = 0
    for mask in (0x01, 0x03, 0x0F, 0xF0, 0xFF, 0x32):                  # 0x32: codes 1, 4, 5 - K = 3 is no power of two
        res = results_with_ties(h, w, mask, seed=h * w + mask)
        assert min(r.min() for r in res.values()) < -0.1 and max(r.max() for r in res.values()) > 1.1
        want = ref.mean_back(res, mask, h, w)
        ties += int(((want.clamp(0, 1) * 255.0) % 1.0 == 0.5).sum())
        ra, rb = halves(res, mask)
        dims = [*(ra.shape[-2:] if ra is not None else (0, 0)), *(rb.shape[-2:] if rb is not None else (0, 0))]
        pa, pb = (None if ra is None else ptr(ra)), (None if rb is None else ptr(rb))
        got = torch.full((B, 3, h, w), float("nan"), device="cuda:0")
        fdn_hip.check(lib.fdn_d4_mean(pa, pb, ptr(got), B, h, w, *dims, mask, st()), "fdn_d4_mean")
        assert torch.equal(got.cpu(), want), f"mean, mask {mask:#x}"
        assert torch.equal(E.mean(ra, rb, mask, h, w), got)
        for bgr in (1, 0):
            post = harness.postprocess(got, h, w, bgr=bool(bgr))
            assert torch.equal(post.cpu(), to_u8(want, bgr))
            for fill in (0xFF, 0x00):
                u8 = torch.full((B, h, w, 3), fill, device="cuda:0", dtype=torch.uint8)
                fdn_hip.check(lib.fdn_d4_post_u8(pa, pb, ptr(u8), B, h, w, *dims, mask, bgr, st()), "fdn_d4_post_u8")
                assert torch.equal(u8, post), f"post_u8, mask {mask:#x}, swap_rb={bgr}, fill {fill:#x}"
            assert torch.equal(E.post_u8(ra, rb, mask, h, w, bgr=bool(bgr)), post)
    print(f"{h}x{w}: {ties} means on a rounding tie")
    assert ties > 20, "no tie reached the rounding"


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------------------
def load(mod, sd):
    mod.load_state_dict(sd, strict=True)
    return mod.to("cuda:0").eval()


@pytest.fixture(scope="module")
def nets(E):
    from basicsr.models.archs.FDN_arch import FDN
    from basicsr.models.archs.LPNet_arch import I_predict_net
    return load(FDN(), fdn_weights(tame=0.03)), load(I_predict_net(), lpnet_weights())


def frames(h, w, seed):
    """textured uint8 frames [B,h,w,3] (CPU), dark on the left and brighter to the right: no symmetry a wrong transform could hide in"""
    g = torch.Generator().manual_seed(seed)
    ramp = torch.linspace(0.15, 0.9, w).view(1, 1, w, 1)
    return (torch.rand(B, h, w, 3, generator=g) * 255 * ramp).to(torch.uint8)


def test_forward_takes_the_transposed_shape(E, nets):
    """96 x 64, the padded transposed 33 x 65 frame, through every kernel of the forward (the generic full-image FFT sizes of
    fourier_fuse included) against the CPU oracle"""
    net, _ = nets
    x = torch.rand(1, 3, 96, 64, generator=torch.Generator().manual_seed(11))
    r = torch.tensor([[0.4]])
    with torch.no_grad():
        got = net(cuda(x), ratio_i=cuda(r), device=torch.device("cuda:0"))[0].cpu()
        want = O.fdn_forward(fdn_weights(tame=0.03), x, r)[0]
    p = O.psnr(got, want)
    print(f"96x64 forward against the oracle: {p:.1f} dB")
    assert p > 100.0


def single_passes(net, img, ratio, bgr):
    """{k: the eager forward on harness.preprocess of the torch-transformed uint8 frames, on the CPU} for all eight codes"""
    from fdn_hip import harness
    out = {}
    with torch.no_grad():
        for k in range(8):
            x = harness.preprocess(cuda(ref.transform(img, k, (1, 2))), bgr=bgr)[0]
            out[k] = net(x, ratio_i=ratio, device=x.device)[0].cpu()
    return out


def compose(passes, e, h, w, bgr):
    """crop -> inverse -> ordered mean (CPU restatement) -> harness.postprocess"""
    from fdn_hip import harness
    return harness.postprocess(cuda(ref.mean_back(passes, ref.MASKS[e], h, w)), h, w, bgr=bgr)


@pytest.mark.parametrize("mode", ["lolblur", "lolv1", "fixed"])
def test_enhance_u8_equals_the_composition_of_single_passes(E, nets, mode):
    from fdn_hip import harness
    net, lp = nets
    h, w, bgr = 33, 65, mode != "lolv1"
    img = frames(h, w, seed=5)
    dimg = cuda(img)
    with torch.no_grad():
        x0 = harness.preprocess(dimg, bgr=bgr)[0]
        if mode == "fixed":
            ratio = cuda(torch.tensor([[0.3], [0.55]]))
        else:
            ratio = (lp(x0) if mode == "lolblur" else harness.lolv1_ratio(x0, lp(x0))).contiguous()
    assert ratio.shape == (B, 1) and ratio[0, 0] != ratio[1, 0]
    kw = dict(bgr=bgr, ratio_mode=mode, ratio=ratio if mode == "fixed" else None)
    passes = single_passes(net, img, ratio, bgr)
    plain = harness.enhance_u8(net, lp, dimg, **kw)
    assert torch.equal(harness.enhance_u8(net, lp, dimg, ensemble=1, **kw), plain)
    if mode != "lolblur":                                              # (there the plain call replays a captured graph)
        assert torch.equal(compose(passes, 1, h, w, bgr), plain)       # the composition with one copy is the plain call
    seen = [plain]
    for e in (2, 4, 8):
        got = harness.enhance_u8(net, lp, dimg, ensemble=e, **kw)
        assert got.dtype == torch.uint8 and got.shape == (B, h, w, 3)
        assert torch.equal(got, compose(passes, e, h, w, bgr)), f"ensemble={e}"
        print(f"{mode}, ensemble={e}: {int((got != plain).sum())} of {got.numel()} bytes differ from the single pass")
        seen.append(got)
    if mode == "lolblur":                                              # batch = 1: one sample per forward, the same bits
        assert torch.equal(harness.enhance_u8(net, lp, dimg, ensemble=8, batch=1, **kw), seen[-1])


def test_validate_u8_with_the_ground_truth_ratio(E, nets):
    from fdn_hip import harness
    from fdn_hip.metrics import calculate_psnr_ssim_u8
    net, _ = nets
    h, w = 33, 65
    lq, gt = frames(h, w, seed=6), frames(h, w, seed=7) // 2 + 100
    dlq, dgt = cuda(lq), cuda(gt)
    with torch.no_grad():
        ratio = harness.gt_ratio(harness.preprocess(dlq)[0], harness.preprocess(dgt)[0]).contiguous()
    want = compose(single_passes(net, lq, ratio, True), 8, h, w, True)
    out, psnr, ssim, r = harness.validate_u8(net, None, dlq, dgt, ratio_mode="gt", ensemble=8)
    assert torch.equal(out, want) and torch.equal(r, ratio)
    wp, ws = calculate_psnr_ssim_u8(want, dgt)
    assert psnr == wp and ssim == ws and len(psnr) == B
    one = harness.validate_u8(net, None, dlq, dgt, ratio_mode="gt", ensemble=1)
    base = harness.validate_u8(net, None, dlq, dgt, ratio_mode="gt")
    assert torch.equal(one[0], base[0]) and one[1] == base[1] and one[2] == base[2] and torch.equal(one[3], base[3])


def test_tiled_route_equals_the_per_tile_composition(E, nets):
    """a 70 x 90 frame in nine 32 x 32 tiles (batch 8: a partial last forward), every tile ensembled as fp32 with the frame's ratio, then
    merged by either blend"""
    from fdn_hip import harness, tiling
    net, lp = nets
    h, w = 70, 90
    img = frames(h, w, seed=8)[0]
    dimg = cuda(img)
    with torch.no_grad():
        tiles, ij = tiling.split_u8(dimg, 32, 32, bgr=True)
        assert tiles.shape == (9, 3, 32, 32)
        r = harness.tile_ratio(lp, dimg, tiles, "lolblur", "frame", bgr=True, batch=8)
        passes = {k: tiling.run_tiles(net, ref.transform(tiles, k, (-2, -1)).contiguous(), r, 8).cpu() for k in range(8)}
        assert torch.equal(passes[0], tiling.run_tiles(net, tiles, r, 8, ensemble=1).cpu())
        for e in (2, 8):
            outs = cuda(ref.mean_back(passes, ref.MASKS[e], 32, 32))
            assert torch.equal(tiling.run_tiles(net, tiles, r, 8, ensemble=e), outs), f"run_tiles, ensemble={e}"
        for blend in ("average", "feather"):
            want = tiling.merge_u8(outs, ij, h, w, bgr=True, blend=blend)
            got = harness.enhance_u8(net, lp, dimg, tile=(32, 32), blend=blend, ensemble=8)
            assert got.shape == (1, h, w, 3) and torch.equal(got[0], want), blend
            frame, ratio = harness.enhance_frame_tiled(net, lp, dimg, (32, 32), blend=blend, ensemble=8)
            assert torch.equal(frame, want) and torch.equal(ratio, r)
            base = harness.enhance_u8(net, lp, dimg, tile=(32, 32), blend=blend)
            assert torch.equal(harness.enhance_u8(net, lp, dimg, tile=(32, 32), blend=blend, ensemble=1), base)
