"""GPU: the feathered tile merge - fdn_tiles_merge_w / fdn_tiles_merge_w_u8, fdn_hip.tiling.merge / merge_u8 / forward_tiled and
fdn_hip.harness.enhance_u8 / validate_u8 with blend="feather", the drivers' --tile-blend, and the one-rank RCCL route.

The reference has no such merge, so the yardstick is the float64 restatement of tests/tile_blend_ref.py on the same float32 weight vectors.
Shapes (frame, tile, overlap asked for; row origins | column origins):

    70 x 90  32 x 32   0   [0, 19, 38] | [0, 29, 58]                       the reference's walk: bands of 13 rows, 3 columns
    70 x 90  32 x 32   8   [0, 19, 38] | [0, 20, 40, 58]                   bands of 13 rows, 12 / 12 / 14 columns
    70 x 90  32 x 32  20   [0, 10, 20, 30, 38] | [0, 12, 24, 36, 48, 58]   4 x 3 = 12 tiles over one pixel, both ramps of a tile meet
    40 x 50  32 x 32   0   [0, 8] | [0, 18]                                an overlap larger than half a tile
    64 x 96  32 x 32   0   [0, 32] | [0, 32, 64]                           no overlap: every weight 1
    32 x 32  32 x 32   0   [0] | [0]                                       one tile

The fp32 bound per value is (K + 3) 2^-23 max|x| with K the tiles over the pixel and max|x| the largest of their values there: the kernel
rounds once per weight product, per product w x, per add of either sum and in the division, all weights are positive, so the numerator is
off by at most (K + 1) 2^-24 sum(w |x|), the denominator by K 2^-24 of itself, the quotient rounds once and the float32 weight product
differs from the restatement's exact one by 2^-24 in both sums: (2 K + 4) 2^-24 max|x| = (K + 2) 2^-23 max|x|, and 2^-23 max|x| to spare.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fdn-tip2025_amd")
if __name__ == "__main__":                                     # the child process of test_feathered_frame_over_a_one_rank_rccl_group
    for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), PKG):
        sys.path.insert(0, p)

from common import fdn_weights, lpnet_weights  # noqa: E402
from tile_blend_ref import merge64  # noqa: E402

from common import poison_uninitialized  # noqa: F401  (autouse, tests/common.py: torch.empty is filled with NaN / the integer maximum)
pytestmark = pytest.mark.gpu

SHAPES = [((70, 90), 0), ((70, 90), 8), ((70, 90), 20), ((40, 50), 0), ((64, 96), 0), ((32, 32), 0)]
IDS = ["70x90-v0", "70x90-v8", "70x90-v20", "40x50", "64x96", "32x32"]
MOST_TILES = {"70x90-v0": 4, "70x90-v8": 4, "70x90-v20": 12, "40x50": 4, "64x96": 1, "32x32": 1}
CROP = 32
# Seeds of the tile values.  The uint8 comparison allows one level where the float64 value lies within the fp32 bound of a rounding tie, and
# asks that under 0.1 % of the pixels do.  Whether they do is a property of the inputs alone (the float64 restatement, no kernel): with
# twelve tiles over a pixel the window is (K + 3) 6.1e-5 wide per value, about 0.14 % of the pixels of 70 x 90 at overlap 20 on average, so
# the seeds are ones at which the restatement meets the share (4 of 6300 pixels there); the test checks that before it asserts.
SEEDS = {((70, 90), 0): 2, ((70, 90), 8): 2, ((70, 90), 20): 35, ((40, 50), 0): 2, ((64, 96), 0): 7, ((32, 32), 0): 1}


@pytest.fixture(scope="module")
def T():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import fdn_hip
    fdn_hip.lib()   # fail loudly if the HIP extension is not built
    from fdn_hip import tiling
    return tiling


def cuda(a):
    return (torch.from_numpy(a) if isinstance(a, np.ndarray) else a).to("cuda:0").contiguous()


def load(mod, sd):
    mod.load_state_dict(sd, strict=True)
    return mod.to("cuda:0").eval()


@pytest.fixture(scope="module")
def nets(T):
    from basicsr.models.archs.FDN_arch import FDN
    from basicsr.models.archs.LPNet_arch import I_predict_net
    return load(FDN(), fdn_weights(tame=0.03)), load(I_predict_net(), lpnet_weights())


def frame(h, w, seed):
    """a textured uint8 frame [h,w,3] (CPU) that gets brighter from left to right, so that tiles differ in their ratios"""
    g = torch.Generator().manual_seed(seed)
    ramp = torch.linspace(0.15, 0.9, w).view(1, w, 1)
    return (torch.rand(h, w, 3, generator=g) * 255 * ramp).to(torch.uint8)


_cases = {}


def case(T, shape):
    """origins, float32 weights, tile values in [-0.2, 1.2] (C = 3) and the float64 restatement of one shape, computed once"""
    if shape not in _cases:
        (h, w), v = shape
        idx = T.tile_origins(h, w, CROP, CROP, v)
        wy, wx = T.feather_weights(idx, CROP, CROP)
        outs = torch.rand(len(idx), 3, CROP, CROP, generator=torch.Generator().manual_seed(SEEDS[shape])) * 1.4 - 0.2
        ref, cover, amax = merge64(outs.numpy(), idx, h, w, wy.numpy(), wx.numpy())
        _cases[shape] = dict(idx=idx, wy=wy, wx=wx, outs=outs, ref=ref, cover=cover, amax=amax, bound=(cover[None] + 3) * 2.0 ** -23 * amax)
    return _cases[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_weighted_merge_against_float64(T, shape, request):
    (h, w), v = shape
    c = case(T, shape)
    ij = cuda(torch.tensor(c["idx"], dtype=torch.int32))
    assert int(c["cover"].max()) == MOST_TILES[request.node.callspec.id]
    assert c["outs"].min() < -0.15 and c["outs"].max() > 1.15
    for C in (1, 3):
        got = T.merge(cuda(c["outs"][:, :C]), ij, h, w, blend="feather")
        assert got.shape == (1, C, h, w) and got.dtype == torch.float32
        err = np.abs(got[0].cpu().numpy().astype(np.float64) - c["ref"][:C])
        worst = float((err / c["bound"][:C]).max())
        print(f"{h}x{w} overlap {v} C={C}: largest error {err.max():.3e}, {worst:.3f} of the bound (K + 3) 2^-23 max|x|")
        assert np.all(err <= c["bound"][:C])

    # uint8: the rounded float64 value; one level off only where 255 x the float64 value lies within 255 x the bound of a rounding tie
    scaled = np.clip(c["ref"], 0.0, 1.0) * 255.0
    want = np.rint(scaled).astype(np.uint8)                                                # half to even, as rintf
    near_tie = np.abs(scaled - np.floor(scaled) - 0.5) <= 255.0 * c["bound"]
    share = float(near_tie.any(axis=0).mean())
    print(f"{h}x{w} overlap {v}: {int(near_tie.any(axis=0).sum())} of {h * w} pixels within the bound of a tie ({100 * share:.3f} %)")
    assert share < 1e-3, "the seeded inputs put too many pixels next to a tie for the comparison to mean anything"
    for bgr in (True, False):
        got = T.merge_u8(cuda(c["outs"]), ij, h, w, bgr=bgr, blend="feather")
        assert got.shape == (h, w, 3) and got.dtype == torch.uint8
        g = got.cpu().numpy().transpose(2, 0, 1)
        g = g[::-1] if bgr else g
        off = g != want
        print(f"{h}x{w} overlap {v} bgr={bgr}: {int(off.sum())} bytes differ from the rounded float64 value")
        assert not np.any(off & ~near_tie)
        assert np.all(np.abs(g.astype(np.int16) - want.astype(np.int16)) <= 1)
        assert float(off.any(axis=0).mean()) < 1e-3


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bit_identities(T, shape):
    """merge_u8(feather) = merge(feather) -> postprocess; blend="average" = the call without the keyword; where no two tiles share a pixel
    every weight is 1 and feather = average, bit for bit"""
    from fdn_hip import harness
    (h, w), v = shape
    c = case(T, shape)
    ij, outs = cuda(torch.tensor(c["idx"], dtype=torch.int32)), cuda(c["outs"])
    merged = T.merge(outs, ij, h, w, blend="feather")
    for bgr in (True, False):
        assert torch.equal(T.merge_u8(outs, ij, h, w, bgr=bgr, blend="feather"), harness.postprocess(merged, h, w, bgr=bgr)[0]), bgr
        assert torch.equal(T.merge_u8(outs, ij, h, w, bgr=bgr, blend="average"), T.merge_u8(outs, ij, h, w, bgr=bgr))
    average = T.merge(outs, ij, h, w)
    assert torch.equal(T.merge(outs, ij, h, w, blend="average"), average)
    assert torch.equal(T.merge(outs[:, :1].contiguous(), ij, h, w, blend="feather")[0, 0], merged[0, 0])       # C = 1 is C = 3's first plane
    if int(c["cover"].max()) == 1:
        assert float(c["wy"].min()) == 1.0 == float(c["wx"].min())
        assert torch.equal(merged, average)
        assert torch.equal(T.merge_u8(outs, ij, h, w, blend="feather"), T.merge_u8(outs, ij, h, w))
    else:
        assert not torch.equal(merged, average)
    with pytest.raises(ValueError, match="blend"):
        T.merge_u8(outs, ij, h, w, blend="linear")


def test_enhance_and_validate_feathered(T, nets):
    """enhance_u8 / validate_u8(tile=(64, 64), overlap=16, blend="feather") on a 96 x 160 frame = split_u8 -> run_tiles -> merge_u8(feather)
    with the ratio the route feeds; forward_tiled(blend="feather") is the same on the fp32 frame"""
    from fdn_hip import harness
    net, lp = nets
    h, w, crop = 96, 160, (64, 64)
    gt = frame(h, w, seed=71)
    lq = (gt.float() * 0.4).to(torch.uint8)
    img = cuda(lq)
    tiles, ij = T.split_u8(img, *crop, bgr=False, overlap=16)
    assert tiles.shape[0] == len(T.tile_origins(h, w, *crop, 16)) == 6           # rows 0, 32; columns 0, 48, 96
    with torch.no_grad():
        r = harness.tile_ratio(lp, img, tiles, "lolblur", "frame", bgr=False)
        outs = T.run_tiles(net, tiles, r, 8)
    want = T.merge_u8(outs, ij, h, w, bgr=False, blend="feather")
    got = harness.enhance_u8(net, lp, img, bgr=False, tile=crop, overlap=16, blend="feather")
    assert got.shape == (1, h, w, 3) and torch.equal(got[0], want)
    plain = harness.enhance_u8(net, lp, img, bgr=False, tile=crop, overlap=16)
    assert torch.equal(plain[0], T.merge_u8(outs, ij, h, w, bgr=False))                   # the default has not moved
    print(f"feathered and averaged frames differ in {int((got != plain).sum())} of {got.numel()} bytes")
    assert torch.equal(harness.enhance_frame_tiled(net, lp, img, crop, bgr=False, overlap=16, blend="feather")[0], want)

    with torch.no_grad():
        rg = harness.tile_ratio(None, img, tiles, "gt", "tile", bgr=False, gt_u8=cuda(gt))
        outs_g = T.run_tiles(net, tiles, rg, 8)
    out, psnr, ssim, ratio = harness.validate_u8(net, None, img, cuda(gt), ratio_mode="gt", bgr=False, tile=crop, ratio_from="tile", overlap=16,
                                                 blend="feather")
    assert torch.equal(out[0], T.merge_u8(outs_g, ij, h, w, bgr=False, blend="feather")) and torch.equal(ratio[0], rg)
    assert len(psnr) == len(ssim) == 1 and np.isfinite(psnr[0])

    x = harness._frame_f32(img, False)
    res = T.forward_tiled(net, lp, x, *crop, ratio=r[:1], overlap=16, blend="feather")
    assert torch.equal(harness.postprocess(res.contiguous(), h, w, bgr=False)[0], want)


def test_command_line_feathered(T, nets, tmp_path):
    """inference_fdn_lolblur.py --tile 64x64 --tile-overlap 16 --tile-blend feather writes the library's bytes"""
    from PIL import Image
    from fdn_hip import harness
    net, lp = nets
    lq = (frame(96, 160, seed=81).float() * 0.4).to(torch.uint8)
    (tmp_path / "lq").mkdir()
    Image.fromarray(lq.numpy()).save(tmp_path / "lq" / "f0.png")
    torch.save({"params": fdn_weights(tame=0.03)}, tmp_path / "fdn.pth")
    torch.save({"params": lpnet_weights()}, tmp_path / "lpnet.pth")
    run = subprocess.run([sys.executable, os.path.join(PKG, "inference_fdn_lolblur.py"), "--fdn", str(tmp_path / "fdn.pth"), "--lpnet",
                          str(tmp_path / "lpnet.pth"), "--input", str(tmp_path / "lq" / "*.png"), "--output", str(tmp_path / "out"), "--tile", "64x64",
                          "--tile-overlap", "16", "--tile-blend", "feather"], capture_output=True, text=True, timeout=600)
    print(run.stdout)
    assert run.returncode == 0, run.stderr
    assert "1 frames ->" in run.stdout and "--tile-overlap" not in run.stderr            # both axes overlap: no hint
    want = harness.enhance_u8(net, lp, cuda(lq), bgr=False, tile=(64, 64), overlap=16, blend="feather")[0]
    assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / "f0.png")), want.cpu().numpy())


def test_feathered_frame_over_a_one_rank_rccl_group(T):
    """enhance_frame_tiled(run=the root's side of run_tiles_sharded, blend="feather") over RCCL with world size 1 equals the direct call; in a
    child process with its own time limit (this file's __main__), since a process group is process-wide state"""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29647", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "sharded feathered == direct: True" in r.stdout


def _rccl_child():
    import torch.distributed as dist
    from basicsr.models.archs.FDN_arch import FDN
    from basicsr.models.archs.LPNet_arch import I_predict_net
    from fdn_hip import harness, tiling
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    net, lp = load(FDN(), fdn_weights(tame=0.03)), load(I_predict_net(), lpnet_weights())
    img = cuda((frame(96, 160, seed=91).float() * 0.4).to(torch.uint8))

    def serve(t, r):
        return tiling.run_tiles(net, t, r, 4)
    kw = dict(bgr=False, overlap=16, batch=4)
    direct = harness.enhance_frame_tiled(net, lp, img, (64, 64), blend="feather", **kw)[0]
    average = harness.enhance_frame_tiled(net, lp, img, (64, 64), **kw)[0]
    out = harness.enhance_frame_tiled(net, lp, img, (64, 64), blend="feather", run=lambda t, r: tiling.run_tiles_root(dist, serve, t, r), **kw)[0]
    also = harness.enhance_frame_tiled(net, lp, img, (64, 64), run=lambda t, r: tiling.run_tiles_root(dist, serve, t, r), **kw)[0]
    tiling.end_serving(dist)
    torch.cuda.synchronize()
    print("sharded feathered == direct:", torch.equal(out, direct) and torch.equal(also, average))
    dist.destroy_process_group()


if __name__ == "__main__":
    _rccl_child()
