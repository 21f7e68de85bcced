"""LPIPS v0.1 restated in torch on the CPU, from its formulas (Zhang et al. 2018; the `lpips` package's LPIPS(version='0.1'), eval mode):

  1. scaling layer per channel: (x - shift_c) / scale_c, shift = (-.030, -.088, -.188), scale = (.458, .448, .450)
  2. the backbone's features after five of its ReLUs (torchvision vgg16().features: relu1_2, relu2_2, relu3_3, relu4_3, relu5_3;
     alexnet().features: ReLUs 1, 4, 7, 9, 11); max-pools without padding, floor mode
  3. per tap and pixel f / (sqrt(sum_c f_c^2) + 1e-10)
  4. d_l = mean_{h,w} sum_c w_{l,c} (f0n_c - f1n_c)^2
  5. LPIPS = sum_l d_l

in float64 (the yardstick) or float32 (what a float32 implementation's own rounding costs).  Also: seeded random weights in the real
file layouts (an lpips.LPIPS state_dict; a torchvision state_dict plus the lpips linear heads) and test images."""
import torch
import torch.nn.functional as F

SHIFT = torch.tensor([-.030, -.088, -.188])          # float32, as lpips' ScalingLayer holds them
SCALE = torch.tensor([.458, .448, .450])

# (torchvision features index, Cin, Cout, kernel, stride, pad) per conv; "P2" / "P3" = MaxPool2d(2, 2) / MaxPool2d(3, 2); "T" = a tap
NETS = {
    "vgg": [(0, 3, 64, 3, 1, 1), (2, 64, 64, 3, 1, 1), "T", "P2", (5, 64, 128, 3, 1, 1), (7, 128, 128, 3, 1, 1), "T", "P2",
            (10, 128, 256, 3, 1, 1), (12, 256, 256, 3, 1, 1), (14, 256, 256, 3, 1, 1), "T", "P2",
            (17, 256, 512, 3, 1, 1), (19, 512, 512, 3, 1, 1), (21, 512, 512, 3, 1, 1), "T", "P2",
            (24, 512, 512, 3, 1, 1), (26, 512, 512, 3, 1, 1), (28, 512, 512, 3, 1, 1), "T"],
    "alex": [(0, 3, 64, 11, 4, 2), "T", "P3", (3, 64, 192, 5, 1, 2), "T", "P3", (6, 192, 384, 3, 1, 1), "T",
             (8, 384, 256, 3, 1, 1), "T", (10, 256, 256, 3, 1, 1), "T"],
}
CHANNELS = {"vgg": [64, 128, 256, 512, 512], "alex": [64, 192, 384, 256, 256]}


def conv_specs(net):
    """[(slice K, index, Cin, Cout, k, stride, pad)]: lpips' slice K holds the convs after K - 1 taps"""
    out, taps = [], 0
    for op in NETS[net]:
        if op == "T":
            taps += 1
        elif not isinstance(op, str):
            out.append((taps + 1,) + op)
    return out


def make_params(net, seed=0):
    """seeded random weights: He-scaled convs with small biases (activations stay alive through the 13 VGG convs), non-negative linear
    heads as trained LPIPS heads are.  -> {"convs": [(w, b)], "lins": [[C]] * 5}, float32"""
    g = torch.Generator().manual_seed(seed)
    convs = []
    for _, _, cin, cout, k, _, _ in conv_specs(net):
        w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
        b = 0.02 * torch.randn(cout, generator=g)
        convs.append((w, b))
    lins = [torch.rand(C, generator=g) * (8.0 / C ** 0.5) for C in CHANNELS[net]]
    return {"convs": convs, "lins": lins}


def lpips_state_dict(net, params, lin_keys=("lin", "lins"), scaling=True):
    """layout (a): an lpips.LPIPS state_dict (net.sliceK.<idx>.*, linK.model.1.weight / lins.K.model.1.weight, scaling_layer.*)"""
    sd = {}
    if scaling:
        sd["scaling_layer.shift"] = SHIFT.clone().reshape(1, 3, 1, 1)
        sd["scaling_layer.scale"] = SCALE.clone().reshape(1, 3, 1, 1)
    for (s, i, *_), (w, b) in zip(conv_specs(net), params["convs"]):
        sd[f"net.slice{s}.{i}.weight"] = w.clone()
        sd[f"net.slice{s}.{i}.bias"] = b.clone()
    sd.update(lin_state_dict(params, lin_keys))
    return sd


def lin_state_dict(params, lin_keys=("lin",)):
    """the lpips linear heads (weights/v0.1/{vgg,alex}.pth has the "lin" form): [1, C, 1, 1] each"""
    sd = {}
    for k, w in enumerate(params["lins"]):
        if "lin" in lin_keys:
            sd[f"lin{k}.model.1.weight"] = w.clone().reshape(1, -1, 1, 1)
        if "lins" in lin_keys:
            sd[f"lins.{k}.model.1.weight"] = w.clone().reshape(1, -1, 1, 1)
    return sd


def torchvision_state_dict(net, params, seed=1):
    """layout (b): a torchvision vgg16 / alexnet state_dict (features.<idx>.*; a small stand-in classifier that the loader ignores)"""
    sd = {}
    for (_, i, *_), (w, b) in zip(conv_specs(net), params["convs"]):
        sd[f"features.{i}.weight"] = w.clone()
        sd[f"features.{i}.bias"] = b.clone()
    g = torch.Generator().manual_seed(seed)
    sd["classifier.1.weight"] = torch.randn(8, 16, generator=g)
    sd["classifier.1.bias"] = torch.zeros(8)
    return sd


def write_weight_files(dirpath, net, seed=0):
    """-> (params, {"lpips": layout (a) with both head forms, "torchvision": layout (b) backbone, "lin": the heads}) as .pth paths"""
    import os
    params = make_params(net, seed)
    paths = {"lpips": os.path.join(dirpath, f"lpips_{net}.pth"), "torchvision": os.path.join(dirpath, f"tv_{net}.pth"),
             "lin": os.path.join(dirpath, f"lin_{net}.pth")}
    torch.save(lpips_state_dict(net, params), paths["lpips"])
    torch.save(torchvision_state_dict(net, params), paths["torchvision"])
    torch.save(lin_state_dict(params), paths["lin"])
    return params, paths


def features(net, params, x):
    """the five taps for x [N,3,H,W] (already through the scaling layer), in x's dtype"""
    taps, ci = [], 0
    for op in NETS[net]:
        if op == "T":
            taps.append(x)
        elif op == "P2":
            x = F.max_pool2d(x, 2, 2)
        elif op == "P3":
            x = F.max_pool2d(x, 3, 2)
        else:
            w, b = params["convs"][ci]
            ci += 1
            x = F.relu(F.conv2d(x, w.to(x.dtype), b.to(x.dtype), stride=op[4], padding=op[5]))
    return taps


def scaling(x, normalize=False):
    """lpips' input handling in float32: normalize=True takes [0, 1] to [-1, 1] (2 x - 1), then the scaling layer"""
    x = x.to(torch.float32)
    if normalize:
        x = 2 * x - 1
    return (x - SHIFT.reshape(1, 3, 1, 1)) / SCALE.reshape(1, 3, 1, 1)


def lpips(net, params, in0, in1, normalize=False, dtype=torch.float64, per_layer=False, prepped=False):
    """LPIPS of the pairs (in0[b], in1[b]) -> [B] (per_layer: [B, 5]) in `dtype`.  The scaling layer in float32 as lpips computes it
    (prepped=True: in0 / in1 are its output already), everything after it in `dtype`."""
    x0 = in0 if prepped else scaling(in0, normalize)
    x1 = in1 if prepped else scaling(in1, normalize)
    x = torch.cat([x0, x1]).to(dtype)
    B = in0.shape[0]
    ds = []
    with torch.no_grad():
        for f, w in zip(features(net, params, x), params["lins"]):
            ds.append(head(f[:B], f[B:], w.to(dtype)))
    d = torch.stack(ds, 1)
    return d if per_layer else d.sum(1)


def head(f0, f1, w):
    """steps 3-4 for one tap: f0, f1 [B,C,H,W], w [C] -> [B]"""
    n0 = f0 / (torch.sqrt((f0 ** 2).sum(1, keepdim=True)) + 1e-10)
    n1 = f1 / (torch.sqrt((f1 ** 2).sum(1, keepdim=True)) + 1e-10)
    return ((n0 - n1) ** 2 * w.reshape(1, -1, 1, 1)).sum(1).mean((1, 2))


def images(B, H, W, seed=0):
    """B structured test images in [0, 1], float32 [B,3,H,W]: gratings, edges and noise"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    out = []
    for _ in range(B):
        f = 0.05 + 0.2 * torch.rand(3, 2, generator=g)
        ph = 6.28 * torch.rand(3, generator=g)
        base = torch.stack([0.5 + 0.3 * torch.sin(f[c, 0] * xx + ph[c]) * torch.cos(f[c, 1] * yy) for c in range(3)])
        base = base + 0.15 * (((xx // 11 + yy // 7) % 2) - 0.5)
        out.append(base + 0.05 * torch.randn(3, H, W, generator=g))
    return torch.stack(out).clamp(0, 1)


def distorted(x, kind, seed=1):
    """'distinct': a 3x3 box blur plus noise of sigma 0.05; 'near': +-1/255 on every value (clamped to [0, 1])"""
    g = torch.Generator().manual_seed(seed)
    if kind == "distinct":
        k = torch.full((3, 1, 3, 3), 1 / 9)
        y = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), k, groups=3)
        y = y + 0.05 * torch.randn(x.shape, generator=g)
    elif kind == "near":
        y = x + (torch.randint(0, 2, x.shape, generator=g).to(torch.float32) * 2 - 1) / 255
    else:
        raise ValueError(kind)
    return y.clamp(0, 1)
