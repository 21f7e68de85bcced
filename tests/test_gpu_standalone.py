"""The stand-alone kernels outside the transformer blocks, each against a plain float64 restatement of the same operation: LPNet's
(7x7 stem, strided 1x1 convs, pools, SE tail, the 1x1 GEMM at pooled-vector shapes), MAR's and the guidance path's small kernels
(narrow 3x3 convs with their sigmoid / residual / post_add epilogue, dw1x1_pad1, scale_batch_, gamma_curve, every fdn_resample mode,
img_mod_maps, dwconv3x3) and the normalisation pair (chan_stats, layernorm_chan).  Whole networks cover these only through one sigmoid
scalar or one PSNR figure; here a failure names the kernel, at sizes that run in seconds.

Bounds (DESIGN.md section 2 has the figures measured against them):
  convs                 relative RMS error < 2e-6 against F.conv2d in float64 (the project's figure for its conv tests)
  element-wise kernels  a first-order rounding bound per element, computed in float64 from the same inputs (u = 2^-24)
  copies / one multiply bit for bit
  conditioning-limited  assert_close_cond: at most 4x the error of the same formula evaluated in fp32 on the CPU, plus a floor
B = 2 wherever a batch exists, so that the plane behind the last one of an image is live memory.  Seeded generators only."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import fdn_oracle as O
from common import assert_close_cond, lpnet_weights, rel_rms

from common import poison_uninitialized  # noqa: F401  (autouse, tests/common.py: torch.empty is filled with NaN / the integer maximum)
pytestmark = pytest.mark.gpu
U = 2.0 ** -24                # unit roundoff of fp32
SENTINEL = -7777.0            # fills the memory a kernel must not write


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import fdn_hip
    fdn_hip.lib()   # fail loudly if the HIP extension is not built
    return fdn_hip


def dev(t):
    return t.to("cuda:0").contiguous()


def load(mod, sd):
    mod.load_state_dict(sd, strict=True)
    return mod.to("cuda:0").eval()


def _rnd(*s, seed):
    return torch.randn(*s, generator=torch.Generator().manual_seed(seed))


def _uni(*s, seed):
    return torch.rand(*s, generator=torch.Generator().manual_seed(seed))


def _act64(v, act):
    from fdn_hip import ACT_GELU, ACT_LEAKY, ACT_NONE, ACT_RELU, ACT_SIGMOID
    return {ACT_NONE: lambda t: t, ACT_LEAKY: lambda t: F.leaky_relu(t, 0.1), ACT_RELU: F.relu, ACT_SIGMOID: torch.sigmoid,
            ACT_GELU: F.gelu}[act](v)


def _conv64(x, w, b, stride, pad, act, res=None, res_before_act=False, post_add=0.0):
    """fdn_conv2d's contract in float64: act(conv + bias [+ res]) [+ res] + post_add"""
    v = F.conv2d(x.double(), w.double(), None if b is None else b.double(), stride=stride, padding=pad)
    if res is not None and res_before_act:
        v = v + res.double()
    v = _act64(v, act)
    if res is not None and not res_before_act:
        v = v + res.double()
    return v + post_add


# ------------------------------------------------------------------------------------------------
# 1. LPNet's kernels
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(16, 64), (17, 66), (37, 71), (5, 3)])
def test_stem_conv7x7s2(L, H, W):
    """conv7x7s2_kernel<3, 16> (LPNet's entry conv with the folded BatchNorm as bias, then ReLU): exactly one 8 x 32 output tile, one more
    row and column of tiles, an odd size and an input smaller than the kernel, against float64; and the kernel's claim of the same
    sums, bit for bit, as the generic kernel (a 17-channel weight whose first 16 rows are the stem's runs conv2d_kernel)."""
    from fdn_hip import ACT_RELU, ops
    x = _rnd(2, 3, H, W, seed=H * 100 + W)
    w, b = _rnd(17, 3, 7, 7, seed=1) / 147 ** 0.5, _rnd(17, seed=2) * 0.2
    got = ops.conv2d(dev(x), dev(w[:16]), dev(b[:16]), stride=2, pad=3, act=ACT_RELU)
    ref = _conv64(x, w[:16], b[:16], 2, 3, ACT_RELU)
    assert got.shape == ref.shape
    e = rel_rms(got.cpu(), ref)
    print(f"stem {H}x{W}: rel_rms {e:.2e}")
    assert e < 2e-6
    generic = ops.conv2d(dev(x), dev(w), dev(b), stride=2, pad=3, act=ACT_RELU)
    assert rel_rms(generic.cpu(), _conv64(x, w, b, 2, 3, ACT_RELU)) < 2e-6
    assert torch.equal(got, generic[:, :16])


@pytest.mark.parametrize("Cin,Cout,k,stride,pad,H,W,act", [
    (16, 32, 1, 2, 0, 25, 24, "relu"),        # SEBlock conv1 / shortcut of LPNet's conv3 stage
    (64, 128, 1, 6, 0, 13, 20, "relu"),       # ... of the conv4 stage: 3 x 4 outputs
    (64, 128, 1, 6, 0, 6, 6, "none"),         # a single output pixel
    (16, 12, 1, 2, 0, 9, 21, "none"),         # the second OCB = 8 group is half full
    (5, 9, 5, 1, 2, 19, 23, "leaky"),         # 437 pixels: two pixel blocks
    (6, 10, 3, 1, 0, 12, 17, "sigmoid"),      # 3 x 3 without padding stays off the 3 x 3 forms
])
def test_conv2d_generic(L, Cin, Cout, k, stride, pad, H, W, act):
    """conv2d_kernel away from 3x3 / pad 1, with bias, against float64."""
    import fdn_hip
    from fdn_hip import ops
    a = getattr(fdn_hip, "ACT_" + act.upper())
    x = _rnd(2, Cin, H, W, seed=Cin + H)
    w, b = _rnd(Cout, Cin, k, k, seed=3) / (Cin * k * k) ** 0.5, _rnd(Cout, seed=4) * 0.2
    got = ops.conv2d(dev(x), dev(w), dev(b), stride=stride, pad=pad, act=a)
    ref = _conv64(x, w, b, stride, pad, a)
    assert got.shape == ref.shape
    e = rel_rms(got.cpu(), ref)
    print(f"conv2d {Cin}->{Cout} k{k} s{stride} p{pad} {H}x{W} {act}: rel_rms {e:.2e}")
    assert e < 2e-6


@pytest.mark.parametrize("before", [True, False])
def test_conv2d_generic_residual(L, before):
    """the residual of conv2d_kernel on either side of the activation (ReLU, so that the side shows in the result)"""
    from fdn_hip import ACT_RELU, ops
    x, res = _rnd(2, 5, 19, 23, seed=5), _rnd(2, 9, 19, 23, seed=6)
    w, b = _rnd(9, 5, 5, 5, seed=7) / 125 ** 0.5, _rnd(9, seed=8) * 0.2
    got = ops.conv2d(dev(x), dev(w), dev(b), stride=1, pad=2, act=ACT_RELU, res=dev(res), res_before_act=before)
    ref = _conv64(x, w, b, 1, 2, ACT_RELU, res, before)
    other = _conv64(x, w, b, 1, 2, ACT_RELU, res, not before)
    assert rel_rms(other, ref) > 0.1                      # the two orders differ, so the wrong one cannot pass
    assert rel_rms(got.cpu(), ref) < 2e-6


@pytest.mark.parametrize("H,W", [(9, 21), (33, 70)])
@pytest.mark.parametrize("Cin", [12, 48])
@pytest.mark.parametrize("Cout", [3, 7])
def test_conv3x3_narrow_options(L, Cout, Cin, H, W):
    """conv3x3_direct_kernel<1, 4> (Cout = 3) and <1, 8> (Cout = 7) with the epilogue of MAR's three output convs (FDN_arch.py:513-521):
    sigmoid, the residual in front of it, post_add.  post_add = 0.25 makes the option visible in the result; with the production value
    1e-8 and one channel's bias at -200 the fp32 sigmoid is exactly 0 there and the output must be float32(1e-8): what the constant is for.
    Per element, the pre-activation sum of n = 9 Cin + 2 terms is off by at most n u sum|terms| to first order, the sigmoid (slope <= 1/4)
    passes a quarter of that on, and exp, the division and the two additions behind it add a few u of the result (8 u allowed)."""
    from fdn_hip import ACT_SIGMOID, ops
    x, res = _rnd(2, Cin, H, W, seed=Cin + Cout + H), _uni(2, Cout, H, W, seed=9)
    w, b = _rnd(Cout, Cin, 3, 3, seed=10) / (9 * Cin) ** 0.5, _rnd(Cout, seed=11) * 0.2
    n = 9 * Cin + 2
    mag = F.conv2d(x.double().abs(), w.double().abs(), b.double().abs(), padding=1)
    for before in (True, False):
        got = ops.conv2d(dev(x), dev(w), dev(b), pad=1, act=ACT_SIGMOID, res=dev(res), res_before_act=before, post_add=0.25).cpu()
        ref = _conv64(x, w, b, 1, 1, ACT_SIGMOID, res, before, 0.25)
        e = rel_rms(got, ref)
        print(f"conv3x3 narrow {Cin}->{Cout} {H}x{W} res_before_act={before}: rel_rms {e:.2e}")
        assert e < 2e-6
        bound = 0.25 * n * U * (mag + res.double()) + 8 * U * ref.abs()
        assert ((got.double() - ref).abs() <= bound).all(), ((got.double() - ref).abs() / bound).max()
    assert rel_rms(_conv64(x, w, b, 1, 1, ACT_SIGMOID, res, True, 0.25), _conv64(x, w, b, 1, 1, ACT_SIGMOID, res, True, 0.0)) > 0.1
    b2 = b.clone()
    b2[Cout - 1] = -200.0
    got = ops.conv2d(dev(x), dev(w), dev(b2), pad=1, act=ACT_SIGMOID, res=dev(res), res_before_act=True, post_add=1e-8).cpu()
    assert rel_rms(got, _conv64(x, w, b2, 1, 1, ACT_SIGMOID, res, True, 1e-8)) < 2e-6
    assert torch.equal(got[:, Cout - 1], torch.full((2, H, W), 1e-8, dtype=torch.float32))
    assert (got > 0).all()


@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (7, 9), (8, 8), (25, 24), (184, 320)])
def test_avgpool3s2(L, H, W):
    """AvgPool2d(3, 2, 1) with count_include_pad=True: eight additions and a division, |err| <= 10 u sum|window| / 9 per element."""
    from fdn_hip import ops
    x = _rnd(2, 4, H, W, seed=H + W)
    got = ops.avgpool3s2(dev(x)).cpu()
    ref = F.avg_pool2d(x.double(), 3, 2, 1)
    assert got.shape == ref.shape
    bound = 10 * U * F.avg_pool2d(x.double().abs(), 3, 2, 1)
    err = (got.double() - ref).abs()
    print(f"avgpool3s2 {H}x{W}: worst err / bound {(err / bound).max():.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("P", [1, 255, 256, 257, 1000])
def test_global_avgpool(L, P):
    """gap_kernel sums ceil(P / 256) values per thread, then eight tree levels, then divides: (ceil(P / 256) + 9) u mean|x| per plane."""
    from fdn_hip import ops
    x = _rnd(5, 1, 1, P, seed=P)
    got = ops.global_avgpool(dev(x)).cpu().view(5).double()
    ref = x.double().view(5, P).mean(1)
    bound = (math.ceil(P / 256) + 9) * U * x.double().abs().view(5, P).mean(1)
    err = (got - ref).abs()
    print(f"global_avgpool P={P}: worst err / bound {(err / bound).max():.3f}")
    assert (err <= bound).all()


def test_global_avgpool_frame(L):
    """3 planes of 736 x 1280 uniform in [0, 1): the shape the harness takes the frame mean from.  The kernel's summation order emulated in
    numpy float32 is off by 1.0e-7 (relative) at this size; a lost element or a wrong divisor shows at the small P above."""
    from fdn_hip import ops
    x = _uni(1, 3, 736, 1280, seed=12)
    got = ops.global_avgpool(dev(x)).cpu().view(3).double()
    ref = x.double().mean(dim=(2, 3)).view(3)
    err = ((got - ref).abs() / ref).max().item()
    print(f"global_avgpool 736x1280: worst relative error {err:.2e}")
    assert err <= 1e-6


def test_se_apply(L):
    """relu(y * gate[plane] + shortcut): one or two roundings, |err| <= 2^-22 (|y g| + |sc|)"""
    from fdn_hip import ops
    y, g, sc = _rnd(2, 3, 7, 11, seed=13), _uni(2, 3, 1, 1, seed=14), _rnd(2, 3, 7, 11, seed=15)
    got = ops.se_apply(dev(y), dev(g), dev(sc)).cpu().double()
    ref = F.relu(y.double() * g.double() + sc.double())
    bound = 2.0 ** -22 * ((y.double() * g.double()).abs() + sc.double().abs())
    assert ((got - ref).abs() <= bound).all()
    assert (ref == 0).any() and (ref > 0).any()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("K,N,act", [(32, 2, "relu"), (64, 4, "relu"), (128, 8, "relu"), (2, 32, "sigmoid"), (4, 64, "sigmoid"),
                                     (8, 128, "sigmoid"), (128, 128, "none"), (128, 1, "sigmoid")])
def test_conv1x1_pooled_vectors(L, B, K, N, act):
    """fdn_conv1x1 at P = 1: the SE MLPs on pooled vectors (K or N in {2, 4, 8}) and LPNet's two linear layers (N = 1 the last)."""
    import fdn_hip
    from fdn_hip import ops
    a = getattr(fdn_hip, "ACT_" + act.upper())
    x = _rnd(B, K, 1, 1, seed=K + N)
    w, b = _rnd(N, K, seed=16) / K ** 0.5, _rnd(N, seed=17) * 0.2 + 0.3
    got = ops.conv1x1(dev(x), dev(w), dev(b), act=a).cpu()
    ref = _act64(F.conv2d(x.double(), w.double().view(N, K, 1, 1), b.double()), a)
    assert got.shape == ref.shape
    e = rel_rms(got, ref)
    print(f"conv1x1 P=1 B={B} {K}->{N} {act}: rel_rms {e:.2e}")
    assert e < 2e-6


@pytest.mark.parametrize("H,W", [(13, 12), (25, 24)])
@pytest.mark.parametrize("N", [16, 32])
def test_conv1x1_lpnet_stage(L, N, H, W):
    """16 -> 16 and 16 -> 32 with the folded BatchNorm as bias and ReLU, at the map sizes of LPNet's first stage for odd frames"""
    from fdn_hip import ACT_RELU, ops
    x = _rnd(2, 16, H, W, seed=N + H)
    w, b = _rnd(N, 16, seed=18) / 4, _rnd(N, seed=19) * 0.2
    got = ops.conv1x1(dev(x), dev(w), dev(b), act=ACT_RELU).cpu()
    ref = F.relu(F.conv2d(x.double(), w.double().view(N, 16, 1, 1), b.double()))
    assert rel_rms(got, ref) < 2e-6


_lpnet_oracle = {}


def _lpnet_ref(which, shape):
    """(x, weights, fp32 scalar, fp32 taps, float64 scalar, float64 taps) of the CPU oracle, once per case"""
    key = (which, shape)
    if key not in _lpnet_oracle:
        sd = lpnet_weights(which) if which else lpnet_weights()
        x = _uni(*shape, seed=shape[2] * 1000 + shape[3]) * 0.3
        t32, t64 = {}, {}
        with torch.no_grad():
            r32 = O.lpnet_forward(sd, x, t32)
            r64 = O.lpnet_forward(O.cast_params(sd, torch.float64), x.double(), t64)
        _lpnet_oracle[key] = (x, sd, r32, t32, r64, t64)
    return _lpnet_oracle[key]


@pytest.mark.parametrize("shape", [(2, 3, 50, 47), (1, 3, 97, 131), (2, 3, 160, 224)])
@pytest.mark.parametrize("which", [None, "lolv1"])
def test_lpnet_taps(L, which, shape):
    """I_predict_net with the real weights at geometries the fixtures do not have: the stem output, the pooled map and the output of each
    stage against the float64 oracle by the 4x-plus-floor policy, and the scalar within 4x the fp32 oracle's own distance to float64
    plus 2e-7 (three times the largest fp32-to-float64 gap of the oracle at these sizes, 6e-8)."""
    from basicsr.models.archs.LPNet_arch import I_predict_net, _fold
    from fdn_hip import ACT_RELU, ops
    x, sd, r32, t32, r64, t64 = _lpnet_ref(which, shape)
    m = load(I_predict_net(), sd)
    got = {}
    # (the module walks the blocks of a stage itself, so the stage's output is its last block's)
    hooks = [getattr(m, n)[-1].register_forward_hook(lambda mod, inp, out, n=n: got.__setitem__(n, out)) for n in ("conv2", "conv3", "conv4")]
    with torch.no_grad():
        r = m(dev(x))
        w, b = _fold(m.conv1[0], m.conv1[1], m._c, "stem")
        got["stem"] = ops.conv2d(dev(x), w, b, stride=2, pad=3, act=ACT_RELU)
        got["pool"] = ops.avgpool3s2(got["stem"])
    for h in hooks:
        h.remove()
    for n in ("stem", "pool", "conv2", "conv3", "conv4"):
        assert got[n].shape == t64[n].shape, n
        e_got, e_ref = assert_close_cond(got[n], t32[n], t64[n], f"lpnet {which} {shape} {n}")
        print(f"lpnet {which} {shape} {n}: rel-RMS err {e_got:.2e} (fp32 oracle {e_ref:.2e})")
    e_got, e_ref = (r.cpu().double() - r64).abs(), (r32.double() - r64).abs()
    print(f"lpnet {which} {shape} scalar: |got - fp64| {e_got.max():.2e}, |fp32 oracle - fp64| {e_ref.max():.2e}")
    assert (e_got <= 4 * e_ref + 2e-7).all(), (e_got, e_ref)


def test_lpnet_use_ori_i(L):
    """use_ori_i=True: gray mean / scalar, against the same quotient of the float64 oracle's values.  The scalar's bound above carried
    through the quotient, plus 1e-6 relative for the gray mean (global_avgpool's bound at frame size and three roundings)."""
    from basicsr.models.archs.LPNet_arch import I_predict_net
    x, sd, r32, _, r64, _ = _lpnet_ref(None, (2, 3, 50, 47))
    m = load(I_predict_net(), sd)
    with torch.no_grad():
        got = m(dev(x), use_ori_i=True).cpu().double()
    xm = x.double().mean(dim=(2, 3))
    ref = (0.2989 * xm[:, 0] + 0.587 * xm[:, 1] + 0.114 * xm[:, 2]).view(-1, 1) / r64
    bound = ref.abs() * ((4 * (r32.double() - r64).abs() + 2e-7) / r64 + 1e-6)
    assert got.shape == ref.shape and ((got - ref).abs() <= bound).all(), (got, ref)


# ------------------------------------------------------------------------------------------------
# 2. MAR's and the guidance path's small kernels
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,H,W", [(12, 9, 13), (24, 5, 255)])
def test_dw1x1_pad1(L, C, H, W):
    """Conv2d(C, C, 1, padding=1, groups=C) (fourier_fuse.fpre[1]): the border is the bias exactly, the interior one multiply and one add;
    W + 2 = 257 needs a second column block."""
    from fdn_hip import ops
    x, w, b = _rnd(2, C, H, W, seed=C), _rnd(C, seed=20), _rnd(C, seed=21)
    got = ops.dw1x1_pad1(dev(x), dev(w), dev(b)).cpu()
    ref = F.conv2d(x.double(), w.double().view(C, 1, 1, 1), b.double(), padding=1, groups=C)
    assert got.shape == ref.shape == (2, C, H + 2, W + 2)
    border = torch.ones(H + 2, W + 2, dtype=torch.bool)
    border[1:-1, 1:-1] = False
    assert torch.equal(got[:, :, border], b.view(1, C, 1).expand(2, C, int(border.sum())))
    bound = 2.0 ** -22 * ((w.double().view(1, C, 1, 1) * x.double()).abs() + b.double().abs().view(1, C, 1, 1))
    assert ((got[:, :, 1:-1, 1:-1].double() - ref[:, :, 1:-1, 1:-1]).abs() <= bound).all()


def test_scale_batch(L):
    """x *= ratio[b] in place: one correctly rounded multiply"""
    from fdn_hip import ops
    x, ratio = _rnd(3, 12, 7, 11, seed=22), _uni(3, seed=23) * 5 + 0.1
    d = dev(x)
    out = ops.scale_batch_(d, dev(ratio))
    assert out is d and torch.equal(d.cpu(), x * ratio.view(3, 1, 1, 1))


def test_gamma_curve(L):
    """1 - (1 - x)^(40 i) (MAR.forward) on x in [0, 1), i = sigmoid(normal) + 1e-8, against the same formula in fp32 on the CPU and in float64
    of the same fp32 inputs; and the exact cases at the ends of the interval."""
    from fdn_hip import ops
    x = _uni(2, 3, 33, 47, seed=24)
    i = torch.sigmoid(_rnd(2, 3, 33, 47, seed=25)) + 1e-8
    got = ops.gamma_curve(dev(x), dev(i))
    ref32 = 1.0 - (1.0 - x) ** (40.0 * i)
    ref64 = 1.0 - (1.0 - x.double()) ** (40.0 * i.double())
    e_got, e_ref = assert_close_cond(got, ref32, ref64, "gamma_curve")
    print(f"gamma_curve: rel-RMS err {e_got:.2e} (fp32 on the CPU {e_ref:.2e})")
    # the ends: x = 0 -> 0; x = 1 with i > 0 -> 1; i = 0 -> 0 for every x of [0, 1] (1 included: 0^0 = 1); no NaN on the grid
    xs = torch.cat([torch.arange(101) / 100.0, torch.tensor([1e-8, 1 - 2.0 ** -24])])
    assert xs[0] == 0 and xs[100] == 1
    is_ = torch.tensor([0.0, 1e-8, 1e-3, 0.25, 0.5, 1.0, 1.0 + 1e-8])
    gx, gi = xs.view(-1, 1).expand(-1, is_.numel()).contiguous(), is_.view(1, -1).expand(xs.numel(), -1).contiguous()
    g = ops.gamma_curve(dev(gx), dev(gi)).cpu()
    assert not torch.isnan(g).any()
    assert (g[0] == 0).all()                          # x = 0
    assert (g[100, 1:] == 1).all()                    # x = 1, i > 0
    assert (g[:, 0] == 0).all()                       # i = 0


def _resample_into(x, out, planes, H, W, mode, r=1):
    """fdn_resample into a buffer of the caller's (ops.resample allocates its own)"""
    from fdn_hip import check, lib, stream
    check(lib().fdn_resample(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(out.data_ptr()), ctypes.c_long(planes), H, W, mode, r, stream()),
          "fdn_resample")


def _guarded(n):
    """n floats between two guard zones of sentinels (the front one keeps the 16-byte alignment)"""
    buf = torch.full((64 + n + 1024,), SENTINEL, device="cuda:0", dtype=torch.float32)
    return buf, buf[64:64 + n]


def _guards_intact(buf, n):
    return bool((buf[:64] == SENTINEL).all()) and bool((buf[64 + n:] == SENTINEL).all())


@pytest.mark.parametrize("shape", [(2, 3, 10, 14), (2, 2, 4, 516)])
def test_resample_nearest_half(L, shape):
    """RS_NEAREST_HALF is a strided copy (258 output columns: a second column block)"""
    from fdn_hip import ops
    x = _rnd(*shape, seed=26)
    assert torch.equal(ops.resample(dev(x), ops.RS_NEAREST_HALF).cpu(), x[..., ::2, ::2])


@pytest.mark.parametrize("shape,r", [((2, 3, 8, 24), 2), ((2, 3, 8, 24), 4), ((2, 2, 8, 1032), 4), ((2, 1, 6, 9), 3)])
def test_resample_pixel_unshuffle(L, shape, r):
    from fdn_hip import ops
    x = _rnd(*shape, seed=27)
    assert torch.equal(ops.resample(dev(x), ops.RS_PIXEL_UNSHUFFLE, r).cpu(), F.pixel_unshuffle(x, r))


def test_resample_chunks(L):
    """More planes than one grid holds (65535): nearest x2 on 65537 planes of 1 x 2, PixelUnshuffle(4) on 4096 planes of 4 x 8 (65536 output
    planes in chunks of 65520) - bit for bit, and nothing written outside the output."""
    from fdn_hip import ops
    x = _rnd(1, 65537, 1, 2, seed=28)
    n = 65537 * 2 * 4
    buf, out = _guarded(n)
    _resample_into(dev(x), out, 65537, 1, 2, ops.RS_NEAREST_X2)
    assert torch.equal(out.cpu().view(1, 65537, 2, 4), F.interpolate(x, scale_factor=2, mode="nearest"))
    assert _guards_intact(buf, n)
    x = _rnd(1, 4096, 4, 8, seed=29)
    n = x.numel()
    buf, out = _guarded(n)
    _resample_into(dev(x), out, 4096, 4, 8, ops.RS_PIXEL_UNSHUFFLE, 4)
    assert torch.equal(out.cpu().view(1, 65536, 1, 2), F.pixel_unshuffle(x, 4))
    assert _guards_intact(buf, n)


def _misaligned(x):
    """the same values 4 bytes off a 16-byte boundary: still contiguous, and fdn_resample takes the scalar kernel"""
    buf = torch.empty(x.numel() + 4, device="cuda:0", dtype=torch.float32)
    v = buf[1:1 + x.numel()].view(x.shape)
    v.copy_(x)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("mode", ["RS_BILINEAR_X2", "RS_BILINEAR_HALF", "RS_NEAREST_X2"])
def test_resample_quad_equals_scalar(L, mode):
    """resample4_kernel (four outputs per thread) and resample_kernel are bit-identical, as the source says.  (This test found the bilinear x2
    pair an ulp apart: the same expression, contracted into FMAs differently per kernel; both now share one blend spelled with fmaf.)"""
    from fdn_hip import ops
    x = dev(_rnd(2, 3, 16, 24, seed=30))
    assert x.data_ptr() % 16 == 0
    assert torch.equal(ops.resample(x, getattr(ops, mode)), ops.resample(_misaligned(x), getattr(ops, mode)))


def test_resample_quad_row_index_past_2p22(L):
    """resample4_kernel finds its row with a float reciprocal below 2^22 (row, quad) indices and an integer division above: one plane of
    2049 x 2050 has 4098 rows of 1025 quads (4.20 M, not a power of two per row), so one launch crosses the threshold.  Against
    F.interpolate in float64 at the figures of test_resample_bilinear_matches_torch, and against the scalar kernel bit for bit."""
    from fdn_hip import ops
    x = _rnd(1, 1, 2049, 2050, seed=31)
    d = dev(x)
    got = ops.resample(d, ops.RS_BILINEAR_X2)
    assert got.shape == (1, 1, 4098, 4100) and 4098 * 1025 > 2 ** 22
    assert torch.equal(got, ops.resample(_misaligned(d), ops.RS_BILINEAR_X2))
    ref = F.interpolate(x.double(), scale_factor=2, mode="bilinear", align_corners=False)
    got = got.cpu()
    assert rel_rms(got, ref) < 1e-6 and (got.double() - ref).abs().max() < 1e-5


def test_resample_refusals(L):
    """odd sizes for the 1/2 modes and H or W that r does not divide: refused on the host, nothing launched, nothing written"""
    from fdn_hip import FdnHipError, ops
    x = dev(_rnd(2, 3, 12, 12, seed=32))
    out = torch.full((2 * 3 * 16 * 12 * 12,), SENTINEL, device="cuda:0", dtype=torch.float32)
    for H, W, mode, r in ((11, 12, ops.RS_NEAREST_HALF, 1), (12, 11, ops.RS_NEAREST_HALF, 1), (11, 12, ops.RS_BILINEAR_HALF, 1),
                          (12, 11, ops.RS_BILINEAR_HALF, 1), (10, 12, ops.RS_PIXEL_UNSHUFFLE, 4), (12, 10, ops.RS_PIXEL_UNSHUFFLE, 4),
                          (12, 12, ops.RS_PIXEL_UNSHUFFLE, 0), (12, 12, 5, 1)):
        with pytest.raises(FdnHipError):
            _resample_into(x, out, 6, H, W, mode, r)
    with pytest.raises(FdnHipError):
        ops.resample(dev(_rnd(2, 3, 9, 12, seed=33)), ops.RS_NEAREST_HALF)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


@pytest.mark.parametrize("H,W", [(9, 13), (33, 65), (32, 64)])
@pytest.mark.parametrize("C", [12, 20, 32])
def test_img_mod_maps(L, C, H, W):
    """conv3_{mul,add}(conv1_{mul,add}(img)) (FDN_arch.py:423) against the two convs in float64; at C = 12 and 20 the last 8-channel group
    is half full, 33 x 65 has one more row and column of tiles than 32 x 64"""
    from fdn_hip import ops
    img = _uni(2, 3, H, W, seed=C + H)
    ws = [_rnd(C, 3, 1, 1, seed=34) / 3 ** 0.5, _rnd(C, 1, 3, 3, seed=35) / 3, _rnd(C, 3, 1, 1, seed=36) / 3 ** 0.5, _rnd(C, 1, 3, 3, seed=37) / 3]
    mul, add = ops.img_mod_maps(dev(img), *[dev(w) for w in ws])
    for got, w1, w3, name in ((mul, ws[0], ws[1], "mul"), (add, ws[2], ws[3], "add")):
        ref = F.conv2d(F.conv2d(img.double(), w1.double()), w3.double(), padding=1, groups=C)
        assert got.shape == ref.shape
        e = rel_rms(got.cpu(), ref)
        print(f"img_mod_maps C={C} {H}x{W} {name}: rel_rms {e:.2e}")
        assert e < 2e-6


@pytest.mark.parametrize("H,W", [(1, 1), (32, 64), (33, 65)])
@pytest.mark.parametrize("act", ["none", "leaky", "relu", "gelu"])
def test_dwconv3x3(L, act, H, W):
    """fdn_dwconv3x3 (in the C ABI, used by no module today) against F.conv2d(groups=C) in float64"""
    import fdn_hip
    from fdn_hip import ops
    a = getattr(fdn_hip, "ACT_" + act.upper())
    x, w = _rnd(2, 5, H, W, seed=H + 38), _rnd(5, 1, 3, 3, seed=39) / 3
    got = ops.dwconv3x3(dev(x), dev(w), act=a).cpu()
    ref = _act64(F.conv2d(x.double(), w.double(), padding=1, groups=5), a)
    assert got.shape == ref.shape
    e = rel_rms(got, ref)
    print(f"dwconv3x3 {act} {H}x{W}: rel_rms {e:.2e}")
    assert e < 2e-6


# ------------------------------------------------------------------------------------------------
# 3. normalisation
# ------------------------------------------------------------------------------------------------
def _stats64(x, groups):
    B, C, H, W = x.shape
    v = x.double().view(B, groups, C // groups, H * W)
    return v.mean(2), 1.0 / torch.sqrt(v.var(2, unbiased=False) + 1e-5)


def _check_stats(x_dev, x_cpu, groups, what):
    from fdn_hip import ops
    B, C, H, W = x_cpu.shape
    st = ops.chan_stats(x_dev, groups=groups).cpu()
    assert st.shape == (B, groups, 2, H * W)
    mean, rstd = _stats64(x_cpu, groups)
    e_m, e_r = rel_rms(st[:, :, 0], mean), rel_rms(st[:, :, 1], rstd)
    print(f"chan_stats {what}: rel_rms mean {e_m:.2e}, rstd {e_r:.2e}")
    assert e_m < 1e-5 and e_r < 1e-5


@pytest.mark.parametrize("H,W", [(24, 40), (9, 21)])          # P % 4 == 0: the float4 form; 189 pixels: the scalar form
@pytest.mark.parametrize("C,groups", [(12, 1), (114, 3), (3, 3), (1, 1)])
def test_chan_stats(L, C, groups, H, W):
    """mean and 1 / sqrt(var + 1e-5) over each channel group against float64; E = 1 has variance 0 and rstd 1 / sqrt(1e-5)"""
    x = _rnd(2, C, H, W, seed=C + H)
    _check_stats(dev(x), x, groups, f"C={C} G={groups} {H}x{W}")
    if C == groups:
        from fdn_hip import ops
        st = ops.chan_stats(dev(x), groups=groups).cpu()
        assert torch.equal(st[:, :, 0].reshape(-1), x.reshape(-1))
        assert (st[:, :, 1].double() - 1e-5 ** -0.5).abs().max() < 1e-5 ** -0.5 * 4 * U


@pytest.mark.parametrize("H,W", [(24, 40), (9, 21)])
def test_chan_stats_channel_slice(L, H, W):
    """a channel slice of a wider tensor: the batch stride is not C * P"""
    t = _rnd(2, 48, H, W, seed=40)
    _check_stats(dev(t)[:, 8:40], t[:, 8:40], 1, f"slice 8:40 of 48 {H}x{W}")


@pytest.mark.parametrize("H,W", [(24, 40), (9, 21)])
def test_chan_stats_offset(L, H, W):
    """x = 1000 + noise: the variance is accumulated around the first channel's value, so no mean^2 cancellation occurs (the naive
    E[x^2] - mean^2 in fp32 is off by orders of magnitude here and fails this bound)."""
    x = 1000.0 + _rnd(2, 12, H, W, seed=41)
    _check_stats(dev(x), x, 1, f"offset 1000 {H}x{W}")
    naive = 1.0 / torch.sqrt(((x * x).mean(1) - x.mean(1) ** 2).clamp_min(0) + 1e-5)
    assert rel_rms(naive, _stats64(x, 1)[1][:, 0].view(2, H, W)) > 1e-3


@pytest.mark.parametrize("H,W", [(24, 40), (9, 21)])
@pytest.mark.parametrize("C", [1, 12, 64])
@pytest.mark.parametrize("offset", [0.0, 1000.0])
def test_layernorm_chan(L, offset, C, H, W):
    """WithBias_LayerNorm over channels, both kernel forms, against O.ln_chan in fp32 (the reference) and float64 (the truth).  With the
    offset the subtraction of the mean loses bits in any fp32 evaluation: the conditioning-aware policy is the right one there."""
    from fdn_hip import ops
    x = offset + _rnd(2, C, H, W, seed=C + H + 42)
    g, b = _rnd(C, seed=43) * 0.2 + 1, _rnd(C, seed=44) * 0.2
    got = ops.layernorm_chan(dev(x), dev(g), dev(b))
    e_got, e_ref = assert_close_cond(got, O.ln_chan(x, g, b), O.ln_chan(x.double(), g.double(), b.double()), f"layernorm_chan C={C} {H}x{W} +{offset}")
    print(f"layernorm_chan C={C} {H}x{W} +{offset}: rel-RMS err {e_got:.2e} (fp32 oracle {e_ref:.2e})")
