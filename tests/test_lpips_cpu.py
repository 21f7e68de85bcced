"""CPU: LPIPS weight loading (fdn_hip.lpips.load_weights), the backbone size arithmetic, the float64 restatement tests/lpips_ref.py and
the pairing / grouping of calculate_lpips.py.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

import lpips_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "fdn-tip2025_amd")
NETS = ("vgg", "alex")


@pytest.fixture(scope="module")
def L():
    from fdn_hip import lpips
    return lpips


@pytest.fixture(scope="module")
def cli():
    sys.path.insert(0, PKG)
    import calculate_lpips
    return calculate_lpips


@pytest.fixture(scope="module", params=NETS)
def files(request, tmp_path_factory):
    net = request.param
    params, paths = R.write_weight_files(str(tmp_path_factory.mktemp(f"w_{net}")), net, seed=3)
    return net, params, paths


def same_packed(a, b):
    assert len(a["convs"]) == len(b["convs"]) and len(a["lins"]) == len(b["lins"]) == 5
    for (wa, ba), (wb, bb) in zip(a["convs"], b["convs"]):
        assert torch.equal(wa, wb) and torch.equal(ba, bb)
    for la, lb in zip(a["lins"], b["lins"]):
        assert torch.equal(la, lb)


def test_layouts_load_to_identical_weights(L, files):
    net, params, paths = files
    a = L.load_weights(net, paths["lpips"])
    b = L.load_weights(net, paths["torchvision"], paths["lin"])
    same_packed(a, b)
    same_packed(a, params)
    for (wa, ba), (_, _, cin, cout, k, _, _) in zip(a["convs"], L.convs(net)):
        assert wa.shape == (cout, cin, k, k) and wa.dtype == torch.float32 and wa.is_contiguous() and ba.shape == (cout,)
    assert [t.numel() for t in a["lins"]] == L.tap_channels(net) == R.CHANNELS[net]
    # (a) without its heads, given as a separate lin file; and from mappings instead of files
    sd = R.lpips_state_dict(net, params, lin_keys=())
    same_packed(L.load_weights(net, sd, paths["lin"]), params)
    same_packed(L.load_weights(net, R.torchvision_state_dict(net, params), R.lin_state_dict(params)), params)


@pytest.mark.parametrize("keys", [("lin",), ("lins",), ("lin", "lins")])
def test_lin_and_lins_forms(L, files, keys):
    net, params, _ = files
    same_packed(L.load_weights(net, R.lpips_state_dict(net, params, lin_keys=keys)), params)


def test_lin_and_lins_must_agree(L, files):
    net, params, _ = files
    sd = R.lpips_state_dict(net, params)
    sd["lins.2.model.1.weight"] = sd["lins.2.model.1.weight"] * 2
    with pytest.raises(L.FdnHipError, match="lins.2.model.1.weight"):
        L.load_weights(net, sd)


def test_conv_spec_matches_the_restatement(L):
    for net in NETS:
        assert [c[:7] for c in L.convs(net)] == R.conv_specs(net)


def _expect(L, net, sd, lin, key):
    with pytest.raises(L.FdnHipError, match=key.replace(".", r"\.")):
        L.load_weights(net, sd, lin)


def test_missing_extra_and_misshapen_keys_are_named(L, files):
    net, params, _ = files
    a = R.lpips_state_dict(net, params)
    s_, i_ = R.conv_specs(net)[-3][:2]
    key = f"net.slice{s_}.{i_}.weight"
    sd = dict(a); del sd[key]
    _expect(L, net, sd, None, key)
    sd = dict(a); del sd["lin4.model.1.weight"]; del sd["lins.4.model.1.weight"]
    _expect(L, net, sd, None, "lin4.model.1.weight")
    sd = dict(a); sd["net.slice1.1.weight"] = torch.zeros(3)                     # a ReLU has no weights
    _expect(L, net, sd, None, "net.slice1.1.weight")
    sd = dict(a); sd["net.slice2.0.bias"] = torch.zeros(64)                      # index 0 belongs to slice 1
    _expect(L, net, sd, None, "net.slice2.0.bias")
    sd = dict(a); k0 = "net.slice1.0.bias"; sd[k0] = torch.zeros(63)
    _expect(L, net, sd, None, k0)
    sd = dict(a); sd["lin1.model.1.weight"] = sd["lin1.model.1.weight"].reshape(-1)
    _expect(L, net, sd, None, "lin1.model.1.weight")
    b, lin = R.torchvision_state_dict(net, params), R.lin_state_dict(params)
    sd = dict(b); del sd["features.0.bias"]
    _expect(L, net, sd, lin, "features.0.bias")
    sd = dict(b); sd["features.30.weight"] = torch.zeros(4)
    _expect(L, net, sd, lin, "features.30.weight")
    sd = dict(b); w = sd["features.0.weight"]; sd["features.0.weight"] = w[:, :2].contiguous()
    _expect(L, net, sd, lin, "features.0.weight")
    ld = dict(lin); ld["lin5.model.1.weight"] = torch.zeros(1, 8, 1, 1)
    _expect(L, net, b, ld, "lin5.model.1.weight")
    ld = dict(lin); del ld["lin0.model.1.weight"]
    _expect(L, net, b, ld, "lin0.model.1.weight")
    with pytest.raises(L.FdnHipError, match="lin_weights"):
        L.load_weights(net, b)                                                       # (b) needs the heads
    with pytest.raises(L.FdnHipError, match="lin_weights"):
        L.load_weights(net, a, lin)                                                  # heads given twice
    with pytest.raises(L.FdnHipError, match="net must be"):
        L.load_weights("squeeze", a)


@pytest.mark.parametrize("key,bad", [("scaling_layer.shift", [-.030, -.088, -.180]), ("scaling_layer.scale", [.5, .5, .5])])
def test_scaling_constants_are_checked(L, files, key, bad):
    net, params, _ = files
    sd = R.lpips_state_dict(net, params)
    sd[key] = torch.tensor(bad).reshape(1, 3, 1, 1)
    _expect(L, net, sd, None, key)
    same_packed(L.load_weights(net, R.lpips_state_dict(net, params, scaling=False)), params)


def test_model_needs_weights_and_a_rocm_device(L, files):
    net, _, paths = files
    with pytest.raises(L.FdnHipError, match="weights"):
        L.LPIPS(net)
    with pytest.raises(L.FdnHipError, match="ROCm"):
        L.LPIPS(net, paths["lpips"], device="cpu")


@pytest.mark.parametrize("H,W", [(16, 16), (31, 31), (64, 64), (96, 160), (250, 333), (736, 1280)])
def test_tap_sizes_follow_the_backbone(L, H, W):
    for net in NETS:
        if net == "alex" and H < 31:
            with pytest.raises(L.FdnHipError, match="too small"):
                L.tap_sizes(net, H, W)
            continue
        x = torch.zeros(1, 3, H, W)
        p = R.make_params(net, 0)
        want = [tuple(f.shape[2:]) for f in R.features(net, p, x)] if H * W <= 96 * 160 else None
        got = L.tap_sizes(net, H, W)
        assert len(got) == 5 and all(h >= 1 and w >= 1 for h, w in got)
        if want is not None:
            assert got == want
    assert L.tap_sizes("vgg", 250, 333) == [(250, 333), (125, 166), (62, 83), (31, 41), (15, 20)]
    assert L.tap_sizes("alex", 250, 333) == [(61, 82), (30, 40), (14, 19), (14, 19), (14, 19)]


def test_too_small_is_refused(L):
    with pytest.raises(L.FdnHipError, match="too small"):
        L.tap_sizes("vgg", 15, 64)
    L.tap_sizes("vgg", 16, 16)
    with pytest.raises(L.FdnHipError, match="too small"):
        L.tap_sizes("alex", 64, 30)


@pytest.mark.parametrize("net", NETS)
def test_restatement_zero_and_symmetric(net):
    p = R.make_params(net, 1)
    x = R.images(2, 48, 40, seed=2)
    y = torch.cat([R.distorted(x[:1], "distinct"), R.distorted(x[1:], "near")])
    assert torch.equal(R.lpips(net, p, x, x, normalize=True), torch.zeros(2, dtype=torch.float64))
    d01 = R.lpips(net, p, x, y, normalize=True)
    d10 = R.lpips(net, p, y, x, normalize=True)
    assert torch.allclose(d01, d10, rtol=1e-12, atol=0)
    assert (d01 > 0).all() and d01[0] > 10 * d01[1]                           # blur + noise scores far above +-1/255
    per = R.lpips(net, p, x, y, normalize=True, per_layer=True)
    assert per.shape == (2, 5) and torch.allclose(per.sum(1), d01, rtol=1e-14)
    f32 = R.lpips(net, p, x, y, normalize=True, dtype=torch.float32)
    assert f32.dtype == torch.float32 and torch.allclose(f32.double(), d01, rtol=1e-4)


def test_calculate_lpips_refuses_unequal_shapes():
    from fdn_hip import FdnHipError, metrics
    with pytest.raises(FdnHipError, match="shapes are different"):
        metrics.calculate_lpips(np.zeros((8, 8, 3), np.uint8), np.zeros((8, 9, 3), np.uint8), weights="unused.pth")


def _png(path, a, mode=None):
    from PIL import Image
    Image.fromarray(a, mode=mode).save(path)


def test_cli_pairs_and_groups(cli, tmp_path):
    g = np.random.default_rng(0)
    gt, rs = tmp_path / "gt", tmp_path / "rs"
    gt.mkdir(); rs.mkdir()
    sizes = {"c": (20, 24), "a": (16, 16), "b": (20, 24), "d": (16, 16), "e": (20, 24)}
    for n, (h, w) in sizes.items():
        _png(gt / f"{n}.png", g.integers(0, 256, (h, w, 3), dtype=np.uint8))
        _png(rs / f"{n}_out.png", g.integers(0, 256, (h, w, 3), dtype=np.uint8))
    pairs = cli.pair_paths(str(gt / "*.png"), str(rs / "*.png"))
    assert [(os.path.basename(a), os.path.basename(b)) for a, b in pairs] == [(f"{n}.png", f"{n}_out.png") for n in "abcde"]
    shapes = [(cli.read_rgb8(a).shape, cli.read_rgb8(b).shape) for a, b in pairs]
    assert shapes[0] == ((16, 16, 3), (16, 16, 3))
    assert cli.group_pairs(shapes, 8) == [[0, 3], [1, 2, 4]]
    assert cli.group_pairs(shapes, 2) == [[0, 3], [1, 2], [4]]
    assert cli.group_pairs(shapes, 1) == [[0], [3], [1], [2], [4]]
    with pytest.raises(ValueError, match="differ in size"):
        cli.group_pairs([((16, 16, 3), (16, 17, 3))], 8)
    os.remove(rs / "e_out.png")
    with pytest.raises(ValueError, match="5 ground-truth images"):
        cli.pair_paths(str(gt / "*.png"), str(rs / "*.png"))
    with pytest.raises(ValueError, match="no ground-truth"):
        cli.pair_paths(str(tmp_path / "none" / "*.png"), str(rs / "*.png"))
    with pytest.raises(SystemExit):
        cli.main(["--gt", str(gt / "*.png"), "--restored", str(rs / "*.png"), "--weights", "unused.pth"])


def test_cli_refuses_what_is_not_8bit_rgb(cli, tmp_path):
    _png(tmp_path / "grey.png", np.zeros((8, 8), np.uint8))
    _png(tmp_path / "rgba.png", np.zeros((8, 8, 4), np.uint8))
    from PIL import Image
    Image.fromarray(np.zeros((8, 8), np.uint16) + 300).save(tmp_path / "grey16.png")
    for n in ("grey", "rgba", "grey16"):
        with pytest.raises(ValueError, match="8-bit RGB"):
            cli.read_rgb8(str(tmp_path / f"{n}.png"))
    _png(tmp_path / "ok.png", np.full((8, 8, 3), 7, np.uint8))
    a = cli.read_rgb8(str(tmp_path / "ok.png"))
    assert a.dtype == np.uint8 and a.shape == (8, 8, 3) and (a == 7).all()
