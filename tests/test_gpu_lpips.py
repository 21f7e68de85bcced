"""LPIPS v0.1 on the GPU (csrc/lpips.hip and fdn_conv2d through fdn_hip.lpips.LPIPS) against the float64 restatement tests/lpips_ref.py,
with seeded random weights in the real file layouts (no trained weights ship here).

The scaling layer and the max-pools are bit for bit torch float32; fdn_lpips_layer on given features matches float64 within 1e-10
relative (an MI355X: 8.7e-15 at worst, C = 512).  Identical inputs give exactly 0; swapping the pair, repeating a call and a pair's place
in a batch leave the bits unchanged.

Whole metric: |gpu - f64| <= 8 S + 1e-7 |f64|, S = sum_l |cpu_f32,l - f64,l| the float32 error of the restatement's five head terms
(what float32 features cost, before those errors cancel in the sum), and within 1e-4 relative on the distinct pairs.  A plain 4 |cpu_f32 -
f64| of the total is no yardstick for the near-identical pairs: the CPU's head errors can cancel to a small fraction of any one of them
(VGG 96x160: total 1.3e-8 relative, S 1.9e-7), and the GPU's float32 convs carry 2-5x the CPU's per-conv error on every route (split-bf16
or fp32 MFMA alike: 3.5e-7 against 1.5e-7 rms relative for 64 -> 64, 9.7e-7 against 1.8e-7 for 512 -> 512), 3e-6 against 5e-7 at relu5_3.
An MI355X gave, relative to f64 (GPU / CPU float32 total / S): distinct pairs 3.4e-9 .. 7.5e-8 (CPU 6.8e-9 .. 5.7e-8); near-identical
pairs VGG 7.6e-7 / 2.1e-8 / 6.3e-7 (64x64), 7.7e-7 / 1.3e-8 / 1.9e-7 (96x160), 1.1e-7 / 6.7e-8 / 1.0e-7 (224x224), 1.1e-7 / 5.2e-8 /
5.2e-8 (250x333), AlexNet 1.2e-7 .. 2.3e-6 (CPU 5.4e-8 .. 8.6e-7, S 1.9e-7 .. 1.0e-6).  What a run gives is printed per case (-s)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_ref as R

from common import poison_uninitialized  # noqa: F401  (autouse, tests/common.py: torch.empty is filled with NaN / the integer maximum)
pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LAYER_RTOL = 1e-10
DISTINCT_RTOL = 1e-4
SIZES = [(64, 64), (96, 160), (224, 224), (250, 333)]


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import fdn_hip
    fdn_hip.lib()   # fail loudly if the HIP extension is not built
    from fdn_hip import lpips
    return lpips


@pytest.fixture(scope="module")
def weights(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("lpips_w"))
    return {net: R.write_weight_files(d, net, seed=5) for net in ("vgg", "alex")}


@pytest.fixture(scope="module")
def models(L, weights):
    return {net: L.LPIPS(net, weights=paths["lpips"], device="cuda:0") for net, (_, paths) in weights.items()}


def cuda(t):
    return t.contiguous().to("cuda:0")


@pytest.mark.parametrize("bgr", [True, False])
def test_prep_u8_bit_exact(L, bgr):
    g = torch.Generator().manual_seed(1)
    img = torch.randint(0, 256, (3, 37, 53, 3), generator=g, dtype=torch.uint8)
    img[0, 0, 0] = torch.tensor([0, 128, 255], dtype=torch.uint8)
    got = L.prep_u8(cuda(img), bgr=bgr).cpu()
    # calculate_lpips.py: imread(...).astype(float32) / 255., img2tensor(bgr2rgb), normalize(mean=.5, std=.5), then the scaling layer
    x = torch.from_numpy(img.numpy().astype(np.float32) / 255.)
    if bgr:
        x = x.flip(-1)
    x = x.permute(0, 3, 1, 2).contiguous()
    x = x.sub(torch.tensor([.5, .5, .5]).view(1, 3, 1, 1)).div(torch.tensor([.5, .5, .5]).view(1, 3, 1, 1))
    want = R.scaling(x, normalize=False)
    assert got.shape == want.shape
    assert torch.equal(got, want)


@pytest.mark.parametrize("normalize", [True, False])
def test_prep_f32_bit_exact(L, normalize):
    x = R.images(2, 29, 41, seed=3)
    if not normalize:
        x = x * 2 - 1
    got = L.prep_f32(cuda(x), normalize=normalize).cpu()
    assert torch.equal(got, R.scaling(x, normalize=normalize))


@pytest.mark.parametrize("k,s", [(2, 2), (3, 2)])
@pytest.mark.parametrize("H,W", [(8, 10), (9, 13), (31, 41), (62, 83)])
def test_maxpool_bit_exact(L, k, s, H, W):
    from fdn_hip import ops
    g = torch.Generator().manual_seed(H * W + k)
    x = torch.randn(3, 5, H, W, generator=g)
    got = ops.maxpool2d(cuda(x), k, s).cpu()
    assert torch.equal(got, F.max_pool2d(x, k, s))


def test_maxpool_refuses_a_window_larger_than_the_plane(L):
    from fdn_hip import FdnHipError, ops
    with pytest.raises(FdnHipError):
        ops.maxpool2d(torch.zeros(1, 1, 2, 5, device="cuda:0"), 3, 2)


@pytest.mark.parametrize("C,H,W", [(64, 37, 53), (512, 9, 7), (192, 61, 82)])
def test_layer_against_float64(L, C, H, W):
    g = torch.Generator().manual_seed(C + H)
    B = 3
    f0 = torch.relu(torch.randn(B, C, H, W, generator=g))
    f1 = torch.relu(torch.randn(B, C, H, W, generator=g))
    f1[1] = f0[1] * (1 + 1e-3 * torch.randn(C, H, W, generator=g))          # near-identical: the expanded form would cancel here
    f0[2, :, 0, :] = 0                                                         # pixels with no activation: the 1e-10 of the norm
    f1[2, :, :, 1] = 0
    w = torch.rand(C, generator=g)
    f = cuda(torch.cat([f0, f1]))
    got = L.layer(f, cuda(w)).cpu()
    want = R.head(f0.double(), f1.double(), w.double())
    rel = ((got - want).abs() / want.abs()).max().item()
    print(f"layer C={C} {H}x{W}: d {want.tolist()}, worst relative error {rel:.2e}")
    assert rel <= LAYER_RTOL
    again = L.layer(f, cuda(w)).cpu()
    assert torch.equal(got, again)
    swapped = L.layer(cuda(torch.cat([f1, f0])), cuda(w)).cpu()
    assert torch.equal(got, swapped)
    base = torch.tensor([0.25, -1.0, 3.0], dtype=torch.float64)
    acc = L.layer(f, cuda(w), out=cuda(base.clone()), accumulate=True).cpu()
    assert torch.equal(acc, base + got)


def check_metric(net, got, per64, per32, kinds, what):
    """got [B] against the restatement's per-head terms per64 (float64) and per32 (float32), [B, 5]"""
    ref64 = per64.sum(1)
    err = (got - ref64).abs()
    err32 = (per32.double().sum(1) - ref64).abs()
    S = (per32.double() - per64).abs().sum(1)
    for i, kind in enumerate(kinds):
        rel, rel32 = (err[i] / ref64[i]).item(), (err32[i] / ref64[i]).item()
        print(f"{net} {what} {kind}: LPIPS {ref64[i].item():.9g}, GPU relative error {rel:.2e}, CPU float32 {rel32:.2e} "
              f"(S {(S[i] / ref64[i]).item():.2e})")
        assert err[i] <= 8 * S[i] + 1e-7 * ref64[i].abs(), (net, what, kind, rel, rel32)
        if kind == "distinct":
            assert rel <= DISTINCT_RTOL and 0.01 < ref64[i].item() < 1.0
        else:
            assert 0 < ref64[i].item() < 0.01


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("net", ["vgg", "alex"])
def test_metric_against_float64(L, weights, models, net, H, W):
    params, _ = weights[net]
    x = R.images(2, H, W, seed=H + W)
    y = torch.cat([R.distorted(x[:1], "distinct", seed=H), R.distorted(x[1:], "near", seed=W)])
    m = models[net]
    got = m(cuda(x), cuda(y), normalize=True).cpu()
    assert got.dtype == torch.float64 and got.shape == (2,)
    per64 = R.lpips(net, params, x, y, normalize=True, per_layer=True)
    per32 = R.lpips(net, params, x, y, normalize=True, per_layer=True, dtype=torch.float32)
    check_metric(net, got, per64, per32, ("distinct", "near"), f"{H}x{W}")
    per = m(cuda(x), cuda(y), normalize=True, per_layer=True).cpu()
    assert per.shape == (2, 5)
    assert torch.allclose(per.sum(1), got, rtol=1e-14, atol=0)
    assert torch.allclose(per, per64, rtol=DISTINCT_RTOL * 10, atol=1e-9)
    # inputs in [-1, 1] (normalize=False) are the same pairs
    assert torch.equal(m(cuda(x * 2 - 1), cuda(y * 2 - 1)).cpu(), got)


@pytest.mark.parametrize("net", ["vgg", "alex"])
def test_invariants(L, models, net):
    m = models[net]
    x = cuda(R.images(8, 64, 96, seed=11))
    y = cuda(R.distorted(x.cpu(), "distinct", seed=12))
    assert torch.equal(m(x, x, normalize=True).cpu(), torch.zeros(8, dtype=torch.float64))
    d = m(x, y, normalize=True).cpu()
    assert torch.equal(m(y, x, normalize=True).cpu(), d)
    assert torch.equal(m(x, y, normalize=True).cpu(), d)
    for b in (0, 3, 7):
        alone = m(x[b:b + 1], y[b:b + 1], normalize=True).cpu()
        assert torch.equal(alone[0], d[b])


def test_refusals(L, models):
    from fdn_hip import FdnHipError
    m = models["alex"]
    a = torch.zeros(1, 3, 64, 64, device="cuda:0")
    with pytest.raises(FdnHipError, match="differ in shape"):
        m(a, torch.zeros(1, 3, 64, 65, device="cuda:0"))
    with pytest.raises(FdnHipError, match="too small"):
        m(torch.zeros(1, 3, 30, 64, device="cuda:0"), torch.zeros(1, 3, 30, 64, device="cuda:0"))
    with pytest.raises(FdnHipError, match="too small"):
        models["vgg"](torch.zeros(1, 3, 64, 15, device="cuda:0"), torch.zeros(1, 3, 64, 15, device="cuda:0"))
    with pytest.raises(FdnHipError):
        m(a.cpu(), a.cpu())


def test_vgg_720p_invariants(L, models):
    m = models["vgg"]
    x = cuda(R.images(1, 736, 1280, seed=21))
    y = cuda(R.distorted(x.cpu(), "distinct", seed=22))
    d = m(x, y, normalize=True).cpu()
    print(f"vgg 736x1280: LPIPS {d.item():.9g}")
    assert torch.isfinite(d).all() and 0.01 < d.item() < 1.0
    assert torch.equal(m(y, x, normalize=True).cpu(), d)
    assert torch.equal(m(x, y, normalize=True).cpu(), d)
    assert m(x, x, normalize=True).item() == 0.0


def test_calculate_lpips_u8(L, weights, models):
    from fdn_hip import metrics
    params, _ = weights["alex"]
    g = np.random.default_rng(4)
    a = (R.images(2, 48, 64, seed=4).permute(0, 2, 3, 1).numpy() * 255).round().astype(np.uint8)
    b = np.clip(a.astype(np.int32) + g.integers(-20, 21, a.shape), 0, 255).astype(np.uint8)
    got = metrics.calculate_lpips(a, b, model=models["alex"])                   # B, G, R
    one = metrics.calculate_lpips(a[1], b[1], model=models["alex"])
    assert isinstance(got, list) and len(got) == 2 and isinstance(one, float) and one == got[1]

    def prep(u):                                                                 # calculate_lpips.py
        x = torch.from_numpy(u.astype(np.float32) / 255.).flip(-1).permute(0, 3, 1, 2).contiguous()
        return R.scaling((x - .5) / .5)
    per64 = R.lpips("alex", params, prep(a), prep(b), prepped=True, per_layer=True)
    per32 = R.lpips("alex", params, prep(a), prep(b), prepped=True, per_layer=True, dtype=torch.float32)
    check_metric("alex", torch.tensor(got, dtype=torch.float64), per64, per32, ("distinct", "distinct"), "uint8 48x64")


def test_cli_end_to_end(L, weights, tmp_path):
    from PIL import Image
    params, paths = weights["alex"]
    gt, rs = tmp_path / "gt", tmp_path / "rs"
    gt.mkdir(); rs.mkdir()
    g = np.random.default_rng(9)
    imgs = []
    for i, (h, w) in enumerate([(48, 64), (40, 40), (48, 64)]):
        a = (R.images(1, h, w, seed=30 + i)[0].permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)
        b = np.clip(a.astype(np.int32) + g.integers(-25, 26, a.shape), 0, 255).astype(np.uint8)
        Image.fromarray(a).save(gt / f"img{i}.png")
        Image.fromarray(b).save(rs / f"img{i}_FDN.png")
        imgs.append((a, b))
    cmd = [sys.executable, os.path.join(ROOT, "fdn-tip2025_amd", "calculate_lpips.py"), "--gt", str(gt / "*.png"), "--restored",
           str(rs / "*.png"), "--net", "alex", "--weights", paths["torchvision"], "--lin", paths["lin"], "--batch", "2"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stderr
    vals = [float(v) for v in re.findall(r"LPIPS: ([0-9.]+)\.\n", out.stdout)]
    avg = float(re.search(r"Average: LPIPS: ([0-9.]+)", out.stdout).group(1))
    assert len(vals) == 3

    def prep(u):                                                                 # R, G, B as decoded (the reference: BGR -> bgr2rgb)
        return R.scaling((torch.from_numpy(u.astype(np.float32) / 255.).permute(2, 0, 1)[None] - .5) / .5)
    want = [R.lpips("alex", params, prep(b), prep(a), prepped=True).item() for a, b in imgs]
    for v, w in zip(vals, want):
        assert abs(v - w) <= 1e-6 + DISTINCT_RTOL * w, (v, w)
    assert abs(avg - sum(want) / 3) <= 1e-6 + DISTINCT_RTOL * avg
