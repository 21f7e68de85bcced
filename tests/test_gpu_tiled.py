"""GPU: tiled inference from uint8 frames - fdn_tiles_gather_u8 / fdn_tiles_merge_u8 (ABI 21), fdn_hip.tiling.split_u8 / merge_u8 /
run_tiles / forward_tiled(ratio=, overlap=), fdn_hip.harness.enhance_u8 / validate_u8 with tile=, the drivers' --tile, and
run_tiles_sharded on a one-rank RCCL group.

The kernels are byte shuffles, one IEEE division and an ordered fp32 sum, so everything up to the network is compared bit for bit: with
a torch restatement on the CPU and with the composition of the four existing entry points.  The tiled uint8 route is compared bit for bit
with forward_tiled on the fp32 frame (same tiles, same sub-batches, same merge).  Shapes (frame, tile, row origins | column origins):

    70 x 90    64 x 64   [0, 6] | [0, 26]            unaligned origins, 4 tiles, heavy overlap
    33 x 65    32 x 32   [0, 1] | [0, 17, 33]        odd origins, three tiles over one pixel along an axis
    100 x 200  64 x 96   [0, 36] | [0, 52, 104]      T = 6 > batch 4: a partial last sub-batch
    96 x 128   64 x 64   [0, 32] | [0, 64]           no overlap along one axis (the shape of test_forward_tiled_matches_oracle)
    96 x 160   96 x 160  [0] | [0]                   T = 1
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fdn-tip2025_amd")
if __name__ == "__main__":                                     # the child process of test_run_tiles_sharded_on_a_one_rank_rccl_group
    for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), PKG):
        sys.path.insert(0, p)

import fdn_oracle as O  # noqa: E402
from common import fdn_weights, lpnet_weights  # noqa: E402

from common import poison_uninitialized  # noqa: F401  (autouse, tests/common.py: torch.empty is filled with NaN / the integer maximum)
pytestmark = pytest.mark.gpu

SHAPES = [((70, 90), (64, 64), 8), ((33, 65), (32, 32), 8), ((100, 200), (64, 96), 4), ((96, 128), (64, 64), 8), ((96, 160), (96, 160), 8)]
IDS = ["70x90", "33x65", "100x200", "96x128", "96x160"]


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


def chw01(img, bgr):
    """uint8 [h,w,3] -> fp32 [3,h,w] R, G, B in [0,1] on the CPU: true division, as numpy's"""
    x = img.to(torch.float32) / 255.0
    return (x.flip(-1) if bgr else x).permute(2, 0, 1).contiguous()


def to_u8(res, bgr):
    """tensor2img on the CPU: fp32 [3,h,w] -> clamp(0,1) * 255, round half to even -> uint8 [h,w,3]"""
    v = (res.clamp(0, 1) * 255.0).round().to(torch.uint8).permute(1, 2, 0)
    return (v.flip(-1) if bgr else v).contiguous()


def gray_mean(x):
    """mean(Grayscale(x)) of [B,3,h,w] on the CPU, the reference's op order (image_restoration_model.py:650-654)"""
    return torch.mean(0.2989 * x[:, 0:1] + 0.587 * x[:, 1:2] + 0.114 * x[:, 2:3], dim=(1, 2, 3)).view(-1, 1)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_u8_tile_kernels_bit_exact(T, shape):
    """fdn_tiles_gather_u8 / fdn_tiles_merge_u8 against a torch restatement on the CPU and against fdn_pre_u8(H = h, W = w) ->
    fdn_tiles_gather and fdn_tiles_merge -> fdn_post_u8(H = h, W = w), both channel orders.  The merge takes values in [-0.2, 1.2] and
    planted (k + 0.5) / 255 (the same in every tile over the pixel) for the half-to-even tie."""
    import fdn_hip
    (h, w), (ch, cw), _ = shape
    lib, st = fdn_hip.lib(), fdn_hip.stream
    idx = O.grids_indices(h, w, ch, cw)[2]
    img = frame(h, w, seed=h + w)
    dimg = cuda(img)
    g = torch.Generator().manual_seed(h * w)
    outs = torch.rand(len(idx), 3, ch, cw, generator=g) * 1.4 - 0.2
    planted = torch.rand(h, w, generator=g) < 0.1
    ties = ((torch.randint(0, 255, (3, h, w), generator=g).float() + 0.5) / 255.0)
    for t, (i, j) in enumerate(idx):
        m = planted[i:i + ch, j:j + cw].expand(3, ch, cw)
        outs[t][m] = ties[:, i:i + ch, j:j + cw][m]
    assert outs.min() < -0.1 and outs.max() > 1.1
    # the merge restated: ordered fp32 sum, division by the count (image_restoration_model.py:315-339), then tensor2img
    acc, cnt = torch.zeros(3, h, w), torch.zeros(1, h, w)
    for t, (i, j) in enumerate(idx):
        acc[:, i:i + ch, j:j + cw] += outs[t]
        cnt[:, i:i + ch, j:j + cw] += 1.0
    avg = acc / cnt
    assert cnt.min() >= 1 and int(((avg.clamp(0, 1) * 255.0) % 1.0 == 0.5).sum()) > 20, "no tie reached the rounding"
    for bgr in (True, False):
        tiles, ij = T.split_u8(dimg, ch, cw, bgr=bgr)
        assert ij.dtype == torch.int32 and ij.cpu().tolist() == [list(t) for t in idx]
        x = chw01(img, bgr)
        want = torch.stack([x[:, i:i + ch, j:j + cw] for i, j in idx])
        assert tiles.shape == want.shape and torch.equal(tiles.cpu(), want), f"gather, bgr={bgr}"
        pre = torch.empty((1, 3, h, w), device="cuda:0")
        fdn_hip.check(lib.fdn_pre_u8(ctypes.c_void_p(dimg.data_ptr()), ctypes.c_void_p(pre.data_ptr()), 1, h, w, h, w, int(bgr), st()), "pre")
        assert torch.equal(pre[0].cpu(), x)
        assert torch.equal(tiles, T.split(pre, ch, cw)[0]), f"gather against the composition, bgr={bgr}"

        got = T.merge_u8(cuda(outs), ij, h, w, bgr=bgr)
        assert got.dtype == torch.uint8 and got.shape == (h, w, 3)
        assert torch.equal(got.cpu(), to_u8(avg, bgr)), f"merge, bgr={bgr}"
        merged = T.merge(cuda(outs), ij, h, w)
        post = torch.empty((1, h, w, 3), device="cuda:0", dtype=torch.uint8)
        fdn_hip.check(lib.fdn_post_u8(ctypes.c_void_p(merged.data_ptr()), ctypes.c_void_p(post.data_ptr()), 1, h, w, h, w, int(bgr), st()), "post")
        assert torch.equal(got, post[0]), f"merge against the composition, bgr={bgr}"


def _compose(T, nets, img, crop, batch, bgr, mode, ratio_from, fixed):
    """the tiled route restated on fp32 tensors: forward_tiled on the unpadded / 255 frame with the ratio the route must feed, then
    tensor2img on the CPU"""
    from fdn_hip import harness
    net, lp = nets
    x = cuda(chw01(img, bgr)[None])
    with torch.no_grad():
        if mode == "fixed":
            r = fixed
        elif ratio_from == "frame":
            xp = harness.preprocess(cuda(img), bgr=bgr)[0]
            r = lp(xp) if mode == "lolblur" else harness.lolv1_ratio(xp, lp(xp))
        elif mode == "lolblur":
            r = None                                            # forward_tiled's own behaviour: LPNet per tile
        else:
            tiles = T.split(x, *crop)[0]
            r = harness.lolv1_ratio(tiles, lp(tiles))
        res = T.forward_tiled(net, lp, x, crop[0], crop[1], batch=batch, ratio=r)
    return to_u8(res[0].cpu(), bgr)


@pytest.mark.parametrize("shape", SHAPES[:4], ids=IDS[:4])
def test_enhance_u8_tiled_equals_the_fp32_composition(T, nets, shape):
    from fdn_hip import harness
    (h, w), crop, batch = shape
    net, lp = nets
    img = frame(h, w, seed=3 * h + w)
    bgr = h % 2 == 1
    n = len(T.tile_origins(h, w, *crop))
    per_tile = torch.linspace(0.2, 0.8, n).view(n, 1)
    for mode in ("lolblur", "lolv1", "fixed"):
        for ratio_from in ("frame", "tile"):
            fixed = None if mode != "fixed" else torch.tensor([[0.37]]) if ratio_from == "frame" else per_tile
            arg = fixed[None] if fixed is not None and ratio_from == "tile" else fixed          # [B,1], or [B,T,1] with one row per tile
            got = harness.enhance_u8(net, lp, cuda(img), bgr=bgr, ratio_mode=mode, ratio=arg, tile=crop, ratio_from=ratio_from, batch=batch)
            assert got.shape == (1, h, w, 3) and got.dtype == torch.uint8
            want = _compose(T, nets, img, crop, batch, bgr, mode, ratio_from, None if fixed is None else cuda(fixed))
            differ = int((got[0].cpu() != want).sum())
            print(f"{h}x{w} {mode} ratio_from={ratio_from}: {differ} of {want.numel()} bytes differ")
            assert differ == 0, (mode, ratio_from)
    # more overlap: more tiles, the same route
    got = harness.enhance_u8(net, lp, cuda(img), bgr=bgr, ratio_mode="fixed", ratio=torch.tensor([[0.37]]), tile=crop, overlap=16, batch=batch)
    x = cuda(chw01(img, bgr)[None])
    res = T.forward_tiled(net, lp, x, crop[0], crop[1], batch=batch, ratio=cuda(torch.tensor([[0.37]])), overlap=16)
    assert len(T.tile_origins(h, w, *crop, overlap=16)) >= n and torch.equal(got[0].cpu(), to_u8(res[0].cpu(), bgr))


def test_one_tile_equals_the_untiled_path(T, nets):
    """96 x 160 with a 96 x 160 tile: T = 1, nothing to pad, nothing to average - the untiled enhance_u8 bit for bit; a frame that "auto" leaves
    whole and a batch take the same routes"""
    from fdn_hip import harness
    net, lp = nets
    img = cuda(torch.stack([frame(96, 160, seed=21), frame(96, 160, seed=22)]))
    assert T.tile_origins(96, 160, 96, 160) == [(0, 0)]
    for mode in ("lolblur", "lolv1", "fixed"):
        ratio = cuda(torch.tensor([[0.3], [0.6]])) if mode == "fixed" else None
        want = harness.enhance_u8(net, lp, img, bgr=False, ratio_mode=mode, ratio=ratio)
        for ratio_from in ("frame", "tile"):
            got = harness.enhance_u8(net, lp, img, bgr=False, ratio_mode=mode, ratio=ratio, tile=(96, 160), ratio_from=ratio_from)
            assert torch.equal(got, want), (mode, ratio_from)
        assert torch.equal(harness.enhance_u8(net, lp, img, bgr=False, ratio_mode=mode, ratio=ratio, tile="auto"), want), mode
        assert torch.equal(harness.enhance_u8(net, lp, img, bgr=False, ratio_mode=mode, ratio=ratio, tile=(736, 1280)), want), mode   # clipped to the frame


def test_ratios(T, nets):
    """ratio_from="frame" feeds every tile what the untiled path feeds, bit for bit; the per-tile ground-truth ratio is the reference's
    mean(gray(tile)) / mean(gray(gt, whole and unpadded)) (image_restoration_model.py:578-586, :650-654 after grids()), restated in float32
    on the CPU, within the rtol 3e-5 that test_gt_ratio holds for the same arithmetic"""
    from fdn_hip import harness
    net, lp = nets
    h, w, crop = 70, 90, (64, 64)
    gt = frame(h, w, seed=31)
    lq = (gt.float() * torch.linspace(0.1, 0.6, w).view(1, w, 1)).to(torch.uint8)
    idx = T.tile_origins(h, w, *crop)
    for mode in ("gt", "lolblur", "lolv1"):
        _, _, _, whole = harness.validate_u8(net, lp, cuda(lq), cuda(gt), ratio_mode=mode, bgr=False)
        _, _, _, tiled = harness.validate_u8(net, lp, cuda(lq), cuda(gt), ratio_mode=mode, bgr=False, tile=crop, ratio_from="frame")
        assert tiled.shape == (1, len(idx), 1) and whole.shape == (1, 1)
        assert torch.equal(tiled[0], whole.expand(len(idx), 1)), mode
    _, _, _, got = harness.validate_u8(net, None, cuda(lq), cuda(gt), ratio_mode="gt", bgr=False, tile=crop, ratio_from="tile")
    x = chw01(lq, False)
    want = gray_mean(torch.stack([x[:, i:i + 64, j:j + 64] for i, j in idx])) / gray_mean(chw01(gt, False)[None])
    print("per-tile gt ratio", got.cpu().reshape(-1).tolist(), "restated", want.reshape(-1).tolist())
    assert got.shape == (1, len(idx), 1) and torch.allclose(got[0].cpu(), want, rtol=3e-5, atol=0)
    assert want.max() / want.min() > 1.3                                                             # the tiles do differ
    with pytest.raises(harness.FdnHipError, match="gray mean 0"):
        harness.validate_u8(net, None, cuda(lq), cuda(torch.zeros_like(gt)), ratio_mode="gt", bgr=False, tile=crop, ratio_from="tile")
    with pytest.raises(harness.FdnHipError, match="untiled path"):
        harness.enhance_u8(net, lp, cuda(frame(20, 90, seed=1)), bgr=False, tile=crop)


def test_forward_tiled_with_a_frame_ratio_matches_oracle(T, nets):
    """forward_tiled(x, 64, 64, ratio=LPNet(whole frame)) at 96 x 128 against the oracle doing the same: grids_split -> fdn_forward with
    the broadcast ratio -> grids_merge.  95 dB is what test_forward_tiled_matches_oracle holds at this frame, tile size and weights
    (measured: 148.1 dB)."""
    net, lp = nets
    x = torch.rand(1, 3, 96, 128, generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        r = lp(cuda(x))
        got = T.forward_tiled(net, lp, cuda(x), 64, 64, ratio=r)
        tiles, idx = O.grids_split(x, 64, 64)
        r_ref = O.lpnet_forward(lpnet_weights(), x)
        outs = O.fdn_forward(fdn_weights(tame=0.03), tiles, r_ref.expand(tiles.shape[0], 1))[0]
    ref = O.grids_merge(outs, idx, 96, 128)
    p = O.psnr(got.cpu(), ref)
    print(f"forward_tiled(ratio=frame) against the oracle: PSNR {p:.2f} dB; ratio {r.item()!r} (oracle {r_ref.item()!r})")
    assert r.shape == (1, 1) and p > 95.0


def test_validate_u8_tiled(T, nets):
    from fdn_hip import harness, metrics
    net, lp = nets
    gt = torch.stack([frame(70, 90, seed=41), frame(70, 90, seed=42)])
    lq = (gt.float() * torch.tensor([0.3, 0.5]).view(2, 1, 1, 1)).to(torch.uint8)
    for mode, ratio_from in (("gt", "tile"), ("gt", "frame"), ("lolblur", "tile")):
        out, psnr, ssim, ratio = harness.validate_u8(net, lp, cuda(lq), cuda(gt), ratio_mode=mode, crop_border=2, bgr=False, tile=(64, 64),
                                                     ratio_from=ratio_from)
        assert out.dtype == torch.uint8 and out.shape == gt.shape and ratio.shape == (2, 4, 1)
        assert (psnr, ssim) == metrics.calculate_psnr_ssim_u8(out, cuda(gt), crop_border=2, bgr=False)
        assert len(psnr) == 2 and all(np.isfinite(psnr)) and all(-1 <= s <= 1 for s in ssim)
        want = harness.enhance_u8(net, None, cuda(lq), bgr=False, ratio_mode="fixed", ratio=ratio, tile=(64, 64))
        assert torch.equal(out, want), (mode, ratio_from)


def _run(script, *args):
    out = subprocess.run([sys.executable, os.path.join(PKG, script), *args], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stderr
    return out


def test_command_lines(T, nets, tmp_path):
    """inference_fdn_lolblur.py and validate_fdn.py with --tile 64x64 on two 70 x 90 frames and one 40 x 72 frame (whose tile is clipped to
    32 x 64): the written frames and the printed scores are the library's; no hint about large frames for small ones"""
    from PIL import Image
    from fdn_hip import harness
    net, lp = nets
    gts = [frame(70, 90, seed=51), frame(70, 90, seed=52), frame(40, 72, seed=53)]
    lqs = [(g.float() * s).to(torch.uint8) for g, s in zip(gts, (0.3, 0.5, 0.4))]
    for d in ("lq", "gt"):
        (tmp_path / d).mkdir()
    for i in range(3):
        Image.fromarray(lqs[i].numpy()).save(tmp_path / "lq" / f"f{i}.png")
        Image.fromarray(gts[i].numpy()).save(tmp_path / "gt" / f"f{i}.png")
    torch.save({"params": fdn_weights(tame=0.03)}, tmp_path / "fdn.pth")
    torch.save({"params": lpnet_weights()}, tmp_path / "lpnet.pth")

    run = _run("inference_fdn_lolblur.py", "--fdn", str(tmp_path / "fdn.pth"), "--lpnet", str(tmp_path / "lpnet.pth"), "--input",
               str(tmp_path / "lq" / "*.png"), "--output", str(tmp_path / "out"), "--tile", "64x64", "--batch", "2")
    assert "3 frames ->" in run.stdout and "--tile auto" not in run.stderr
    for i in range(3):
        want = harness.enhance_u8(net, lp, cuda(lqs[i]), bgr=False, tile=(64, 64), batch=2)[0]
        assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / f"f{i}.png")), want.cpu().numpy()), i

    run = _run("validate_fdn.py", "--fdn", str(tmp_path / "fdn.pth"), "--lq", str(tmp_path / "lq" / "*.png"), "--gt", str(tmp_path / "gt" / "*.png"),
               "--tile", "64x64", "--batch", "2", "--csv", str(tmp_path / "scores.csv"))
    assert "--tile auto" not in run.stderr
    csv = (tmp_path / "scores.csv").read_text().splitlines()
    assert csv[0] == "frame,psnr,ssim,ratio" and len(csv) == 4
    for i, line in enumerate(csv[1:]):
        _, psnr, ssim, ratio = harness.validate_u8(net, None, cuda(lqs[i]), cuda(gts[i]), ratio_mode="gt", bgr=False, tile=(64, 64), ratio_from="tile",
                                                   batch=2)
        f, p, s, r = line.rsplit(",", 3)
        assert f.endswith(f"f{i}.png") and float(p) == psnr[0] and float(s) == ssim[0]
        assert [float(v) for v in r.split(";")] == ratio.reshape(-1).cpu().tolist() and ratio.shape == (1, 4, 1)
        assert f"PSNR: {psnr[0]:.6f} dB, \tSSIM: {ssim[0]:.6f}" in run.stdout


def test_run_tiles_sharded_on_a_one_rank_rccl_group(T):
    """scatter_uneven -> run_tiles -> gather_uneven over RCCL with world size 1 equals run_tiles; in a child process with its own time
    limit (this file's __main__), since a process group is process-wide state"""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29643", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "sharded == direct: True" in r.stdout


def _rccl_child():
    import torch.distributed as dist
    from basicsr.models.archs.FDN_arch import FDN
    from fdn_hip import tiling
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    net = load(FDN(), fdn_weights(tame=0.03))
    g = torch.Generator().manual_seed(61)
    tiles, ratio = cuda(torch.rand(5, 3, 32, 64, generator=g)), cuda(torch.rand(5, 1, generator=g) * 0.6 + 0.2)
    direct = tiling.run_tiles(net, tiles, ratio, batch=4)
    out = tiling.run_tiles_sharded(dist, lambda t, r: tiling.run_tiles(net, t, r, batch=4), 5, tiles[:1], tiles, ratio)
    also = tiling.run_tiles_root(dist, lambda t, r: tiling.run_tiles(net, t, r, batch=4), tiles, ratio)
    tiling.end_serving(dist)
    torch.cuda.synchronize()
    print("sharded == direct:", torch.equal(out, direct) and torch.equal(also, direct) and bool(torch.isfinite(direct).all()))
    dist.destroy_process_group()


if __name__ == "__main__":
    _rccl_child()
