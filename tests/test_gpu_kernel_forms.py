"""GPU: the compiled kernel instantiations that no other module of the suite launched (profiles/kernel_coverage_before.txt: a kernel trace of
the whole GPU suite against the library's kernel-descriptor symbols, tools/kernel_coverage.py).  Each case hands an entry point the smallest
argument set that selects the form - a dtype pair, a null prologue, a view that is only 4-byte aligned where the launcher documents a scalar
fallback, an H or W that factors onto that plan - and holds the result to a float64 restatement of the operation at the bound the suite
already applies to that entry point's other forms.  Bit-identity with a sibling form is asserted only where the two differ in load or store
width alone.  tests/kernel_table.txt records, per kernel, the test files that launch it; tests/test_kernel_table_cpu.py holds the table to
the build.
"""
import ctypes

import pytest
import torch

import fdn_oracle as O
from common import assert_close_cond, rel_rms
from test_gpu_geometry import _core, _mid

from common import poison_uninitialized  # noqa: F401  (autouse, tests/common.py: torch.empty is filled with NaN / the integer maximum)
pytestmark = pytest.mark.gpu
F = torch.nn.functional
D = torch.float64
BF = torch.bfloat16
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import fdn_hip
    fdn_hip.lib()
    from fdn_hip import ops
    return ops


def dev(t):
    return t.to("cuda:0").contiguous()


def _rnd(*s, seed):
    return torch.randn(*s, generator=torch.Generator().manual_seed(seed))


def _misaligned(x):
    """the same values 4 bytes off a 16-byte boundary, still contiguous (as in test_gpu_standalone.py)"""
    buf = torch.empty(x.numel() + 4, device="cuda:0", dtype=torch.float32)
    v = buf[1:1 + x.numel()].view(x.shape)
    v.copy_(x)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


# ---------------------------------------------------------------------------------------------------------------------------------
# fdn_fdsa_core: fdsa_core_kernel<false>, the scalar halo fetch (hidden not 16-byte aligned; W % 8 == 0 always holds)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,H,W", [(11, 16, 40), (5, 24, 72)])
def test_fdsa_core_scalar_halo(ops, E, H, W):
    """<false> and <true> differ in how the halo reaches LDS (dwords against float4 + edge dwords); the stencil, the transforms and the
    stores read LDS with one spelling, so the two are bit-identical, and the scalar form is held to float64 like every other fdsa_core case."""
    B = 2
    h = _rnd(B, 4 * E, H, W, seed=1)
    dw, fw = _rnd(4 * E, 1, 3, 3, seed=5) / 3, _rnd(E, 1, 1, 8, 5, seed=6) * 0.2 + 1.0
    truth, ref32 = _core(h.to(D), dw.to(D), fw.to(D)), _core(h, dw, fw)
    hd, dwd, fwd = dev(h), dev(dw), dev(fw)
    got = ops.fdsa_core(_misaligned(hd), dwd, fwd)
    assert_close_cond(got, ref32, truth, f"fdsa_core scalar halo E={E}")
    assert torch.equal(got, ops.fdsa_core(hd, dwd, fwd))


def test_fdsa_core_refuses_a_misaligned_out(ops):
    """the launcher falls back for `hidden` only: an `out` that is not 16-byte aligned is an invalid argument, and nothing is written"""
    import fdn_hip
    B, E, H, W = 1, 3, 8, 16
    hd, dwd, fwd = dev(_rnd(B, 4 * E, H, W, seed=1)), dev(_rnd(4 * E, 1, 3, 3, seed=2)), dev(_rnd(E, 1, 1, 8, 5, seed=3))
    out = _misaligned(torch.full((B, 4 * E, H, W), SENTINEL, device="cuda:0"))
    rc = fdn_hip.lib().fdn_fdsa_core(_ptr(hd), _ptr(dwd), _ptr(fwd), _ptr(out), B, E, H, W, fdn_hip.stream())
    torch.cuda.synchronize()
    assert rc == 1 and bool((out == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# fp32 in, bf16 out: fdffn_mid_kernel<false, false, true>, dw_gate_kernel<true | false, false, true>
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hd,H,W", [(13, 16, 40), (9, 24, 72)])
def test_fdffn_mid_f32_in_bf16_out(ops, Hd, H, W):
    """storage only (test_gpu_bf16.py): the bf16 result is round-to-nearest-even of the fp32 form's, which is held to float64"""
    B = 2
    x = _rnd(B, Hd, H, W, seed=1)
    w0, w2 = _rnd(Hd, 1, 3, 3, seed=5) / 3, _rnd(Hd, 1, 3, 3, seed=6) / 3
    fa, fp = _rnd(Hd, 1, 1, 8, 5, seed=7) * 0.2 + 1, _rnd(Hd, 1, 1, 8, 5, seed=8) * 0.5
    truth, ref32 = _mid(x.to(D), w0.to(D), w2.to(D), fa.to(D), fp.to(D)), _mid(x, w0, w2, fa, fp)
    xd, a = dev(x), [dev(t) for t in (w0, w2, fa, fp)]
    o32 = ops.fdffn_mid(xd, *a)
    o16 = ops.fdffn_mid(xd, *a, out_dtype=BF)
    assert_close_cond(o32, ref32, truth, f"fdffn_mid Hd={Hd}")
    assert o16.dtype == BF and torch.equal(o16, o32.to(BF))


@pytest.mark.parametrize("C,H,W,quad", [(7, 16, 40, True), (7, 16, 40, False), (5, 12, 70, False)])
def test_dwconv_gate_f32_in_bf16_out(ops, C, H, W, quad):
    """quad: W % 4 == 0 and a 16-byte aligned x (16-byte halo loads); otherwise the dword form, by a 4-byte aligned view or by W % 4 != 0.
    The two fp32 forms differ in the halo fetch alone (dw_gate_rows reads LDS): bit-identical."""
    B = 2
    x, wg = _rnd(B, C, H, W, seed=1), _rnd(2 * C, 1, 3, 3, seed=9) / 3
    x1, x2 = F.conv2d(x.to(D), wg.to(D), padding=1, groups=C).chunk(2, dim=1)
    ref = F.gelu(x1) * x2
    xd, wd = dev(x), dev(wg)
    xs = xd if quad or W % 4 else _misaligned(xd)
    g32 = ops.dwconv_gate(xs, wd)
    g16 = ops.dwconv_gate(xs, wd, out_dtype=BF)
    assert rel_rms(g32.cpu(), ref) < 2e-6                        # the bound of test_bf16_gate_dword_forms
    assert g16.dtype == BF and torch.equal(g16, g32.to(BF))
    if xs is not xd:
        assert torch.equal(g32, ops.dwconv_gate(xd, wd))


# ---------------------------------------------------------------------------------------------------------------------------------
# fdn_fdsa_fused without the LayerNorm prologue, fp32 and bf16 out, at the four widths: fdsa_fused_kernel<C, false, ., 0>
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,H,W", [(24, 16, 40), (32, 24, 72), (48, 16, 40), (64, 16, 40)])
def test_fdsa_fused_without_layernorm(ops, C, H, W):
    """against float64 with the conditioning-aware bound of test_fdsa_fused_equals_unfused (reference: fdn_conv1x1 -> fdn_fdsa_core); the bf16
    result is round-to-nearest-even of the fp32 one"""
    B, E = 2, int(C * 1.2)
    x = _rnd(B, C, H, W, seed=1) * 1.5 + 0.3
    w = _rnd(4 * E, C, seed=2) / C ** 0.5
    dw, fw = _rnd(4 * E, 1, 3, 3, seed=5) / 3, _rnd(E, 1, 1, 8, 5, seed=6) * 0.2 + 1.0
    xd, wd, dwd, fwd = dev(x), dev(w), dev(dw), dev(fw)
    wpk = ops.fdsa_pack(wd, None, None)
    ref = ops.fdsa_core(ops.conv1x1(xd, wd), dwd, fwd)
    got = ops.fdsa_fused(xd, None, wpk, dwd, fwd)
    got16 = ops.fdsa_fused(xd, None, wpk, dwd, fwd, out_dtype=BF)
    truth = _core(F.conv2d(x.to(D), w.to(D).view(4 * E, C, 1, 1)), dw.to(D), fw.to(D))
    assert_close_cond(got, ref, truth, f"fdsa_fused C={C} without LayerNorm")
    assert got16.dtype == BF and torch.equal(got16, got.to(BF))


# ---------------------------------------------------------------------------------------------------------------------------------
# fdn_fdsa_fused_tail without the LayerNorm prologue and with the following project_in: fdsa_fused_kernel<24 | 32, false, false, 3>,
# <64, false, false, 4>
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,H,W", [(2, 24, 16, 40), (2, 32, 24, 72), (2, 64, 16, 40)])
def test_fdsa_tail_project_in_without_layernorm(ops, B, C, H, W):
    """the contract of the one-launch route (tests/test_gpu_fdsa_tail.py): bit-identity with fdn_fdsa_fused + fdn_fdsa_out + fdn_conv1x1, each of
    which is held to float64 on its own (test_fdsa_fused_without_layernorm above for this prologue)"""
    from test_gpu_fdsa_tail import _case, _one, _pair
    d = _case(ops, B, C, H, W, seed=5 * C + H + W, ln=False, res=True, edge=H >= 24)
    ya, sa, ha = _pair(ops, d, pin=True)
    yb, sb, hb = _one(ops, d, pin=True)
    torch.cuda.synchronize()
    assert torch.isfinite(yb).all() and torch.isfinite(hb).all()
    assert torch.equal(ya, yb) and torch.equal(sa, sb)
    assert hb.shape == ha.shape and torch.equal(ha, hb), f"h: max |diff| {(ha - hb).abs().max().item():.3e}"


# ---------------------------------------------------------------------------------------------------------------------------------
# fdn_fdsa_out at level 2 off the default forms: fdsa_out_kernel<38, 2> (fp32 MFMA, no 16-byte lanes: odd P) and
# fdsa_out_vec_kernel<38, 2, false, true, 2, 4, false> (bf16 storage in, the fp32-MFMA pixel-pair form of fdn_set_matrix_pipe(2))
# ---------------------------------------------------------------------------------------------------------------------------------
def _fdsa_out_case(E, N, P, seed):
    B = 2
    g = torch.Generator().manual_seed(seed)
    o, w = torch.randn(B, 4 * E, P, generator=g), torch.randn(N, 3 * E, generator=g) / (3 * E) ** .5
    g3, b3, res = torch.randn(3 * E, generator=g), torch.randn(3 * E, generator=g), torch.randn(B, N, P, generator=g)
    return o, w, g3, b3, res


def _fdsa_out_ref(o, w, g3, b3, res):
    """three LayerNorms * v_value, project_out, residual (FDN_arch.py:633-639, :671) in float64, as test_gpu_geometry.py restates it"""
    E = o.shape[1] // 4
    od, v = o.to(D), o.to(D)[:, 3 * E:]
    parts = []
    for k in range(3):
        og = od[:, k * E:(k + 1) * E]
        mu, var = og.mean(1, keepdim=True), og.var(1, unbiased=False, keepdim=True)
        parts.append(((og - mu) / torch.sqrt(var + 1e-5) * g3[k * E:(k + 1) * E].to(D)[None, :, None] + b3[k * E:(k + 1) * E].to(D)[None, :, None]) * v)
    return torch.einsum("nk,bkp->bnp", w.to(D), torch.cat(parts, 1)) + res.to(D)


def _fdsa_out_run(o_dev, w, g3, b3, res, bf16):
    import fdn_hip
    B, E4, P = o_dev.shape
    N = w.shape[0]
    out = torch.full((B, N, P), float("nan"), device="cuda:0")
    st = torch.full((B, 2, P), float("nan"), device="cuda:0")
    rc = fdn_hip.lib().fdn_fdsa_out(_ptr(o_dev), _ptr(w), _ptr(g3), _ptr(b3), _ptr(res), _ptr(out), _ptr(st), B, E4 // 4, N, P, int(bf16), fdn_hip.stream())
    assert rc == 0, rc
    return out.cpu(), st.cpu()


def _assert_fdsa_out(out, st, ref):
    assert rel_rms(out, ref) < 2e-6                             # the bounds of test_fdsa_out_geometry
    assert rel_rms(st[:, 0], ref.mean(1)) < 1e-5 and rel_rms(st[:, 1], 1 / torch.sqrt(ref.var(1, unbiased=False) + 1e-5)) < 1e-5


def test_fdsa_out_level2_without_16_byte_lanes(ops):
    """E = 76, N = 64 on an odd pixel count (13 x 21 = 273: three 128-pixel tiles per image, the last one ragged)"""
    o, w, g3, b3, res = _fdsa_out_case(76, 64, 273, seed=21)
    out, st = _fdsa_out_run(dev(o), dev(w), dev(g3), dev(b3), dev(res), False)
    _assert_fdsa_out(out, st, _fdsa_out_ref(o, w, g3, b3, res))


def test_fdsa_out_level2_bf16_in_on_the_fp32_mfma_form(ops):
    """storage only: reading bf16 equals the fp32 form (the "vec-narrow" case of test_fdsa_out_geometry) fed the stored values, bit for bit, and
    that result is held to float64 of the stored values; 12 x 22 = 264 pixels: two 256-pixel tiles per image"""
    import fdn_hip
    o, w, g3, b3, res = _fdsa_out_case(76, 64, 264, seed=22)
    o = o.to(BF).float()
    a = [dev(t) for t in (w, g3, b3, res)]
    try:
        fdn_hip.set_matrix_pipe("bf16-narrow")
        out32, st32 = _fdsa_out_run(dev(o), *a, False)
        out16, st16 = _fdsa_out_run(dev(o).to(BF), *a, True)
    finally:
        fdn_hip.set_matrix_pipe("bf16")
    _assert_fdsa_out(out32, st32, _fdsa_out_ref(o, w, g3, b3, res))
    assert torch.equal(out16, out32) and torch.equal(st16, st32)


# ---------------------------------------------------------------------------------------------------------------------------------
# fdn_conv1x1: the instantiations no other case reaches.  Each case asserts the route (csrc/conv1x1_route.hpp) before it runs, and
# tests/test_host_cpu.py pins it without a GPU.  13 x 21 = 273 pixels: no 16-byte lanes, three 128-pixel or two 256-pixel tiles per image,
# the last one ragged; 12 x 22 = 264: the pixel-pair forms, two 256-pixel tiles.
# ---------------------------------------------------------------------------------------------------------------------------------
CONV1X1 = {   # name: K, N, H, W, prologue, epilogue, act, want_stats, x stored as bf16, the route
    "early_ln_1": (32, 32, 13, 21, "ln", "res", 0, False, 0, "generic<1,ln,4,1>"),
    "muladd_no_epilogue_1": (32, 32, 13, 21, "muladd", None, 0, False, 0, "generic<1,muladd,8,0>"),
    "early_ln_2": (48, 64, 13, 21, "ln", "res", 0, False, 0, "generic<2,ln,4,1>"),
    "ln3_2": (114, 64, 13, 21, "ln3", "res", 0, True, 0, "generic<2,ln3,4,0>"),
    "muladd_no_epilogue_2": (48, 64, 13, 21, "muladd", None, 0, False, 0, "generic<2,muladd,8,0>"),
    "ln_3": (64, 96, 13, 21, "ln", None, 0, False, 0, "generic<3,ln,4,0>"),
    "ln3_3": (114, 80, 13, 21, "ln3", None, 1, False, 0, "generic<3,ln3,4,0>"),
    "ln3_4": (90, 112, 13, 21, "ln3", "res", 0, True, 0, "generic<4,ln3,4,0>"),
    "smallk_2_muladd": (48, 128, 13, 21, "muladd", "muladd", 0, False, 0, "smallk<2,muladd>"),
    "narrow_1_bf16": (24, 16, 12, 22, None, "res", 0, True, 1, "narrow_tail<1,xbf=1>"),
    "kstream_1": (100, 24, 12, 22, None, "res", 0, True, 0, "kstream_vec<1,xbf=0>"),
    "kstream_1_bf16": (100, 24, 12, 22, None, "res", 0, True, 1, "kstream_vec<1,xbf=1>"),
    "kstream_3": (100, 80, 12, 22, None, "res", 1, True, 0, "kstream_vec<3,xbf=0>"),
    "kstream_3_bf16": (100, 80, 12, 22, None, "res", 1, True, 1, "kstream_vec<3,xbf=1>"),
}


@pytest.mark.parametrize("name", list(CONV1X1))
def test_conv1x1_forms(ops, name):
    from common import conv1x1_route_name
    K, N, H, W, pro, epi, act, want_stats, xbf, route = CONV1X1[name]
    B = 2
    x, w = _rnd(B, K, H, W, seed=1) * 1.5 + 0.3, _rnd(N, K, seed=2) / K ** 0.5
    if xbf:
        x = x.to(BF).float()                                    # the values the kernel reads
    bias = _rnd(N, seed=3) * 0.1
    xs, xd = dev(x), x.to(D)
    kw = {}
    if pro == "ln":
        g, b_ = _rnd(K, seed=4), _rnd(K, seed=5)
        xin = O.ln_chan(xd, g.to(D), b_.to(D))
        kw["ln"] = (ops.chan_stats(xs), dev(g), dev(b_))
    elif pro == "ln3":
        E = K // 3
        g, b_, vv = _rnd(K, seed=4), _rnd(K, seed=5), _rnd(B, E, H, W, seed=6)
        xin = torch.cat([O.ln_chan(xd[:, i * E:(i + 1) * E], g[i * E:(i + 1) * E].to(D), b_[i * E:(i + 1) * E].to(D)) * vv.to(D)
                         for i in range(3)], 1)
        kw["ln3_gate"] = (ops.chan_stats(xs, groups=3), dev(g), dev(b_), dev(vv))
    elif pro == "muladd":
        g, b_, x1 = _rnd(K, seed=4), _rnd(K, seed=5), _rnd(B, K, H, W, seed=6)
        xin = O.ln_chan(xd, g.to(D), b_.to(D)) * x1.to(D) + x1.to(D)
        kw["ln_muladd"] = (ops.chan_stats(xs), dev(g), dev(b_), dev(x1))
    else:
        xin = xd
    ref = F.conv2d(xin, w.to(D).view(N, K, 1, 1), bias.to(D))
    if act == 1:
        ref = F.leaky_relu(ref, 0.1)
    if epi == "res":
        r = _rnd(B, N, H, W, seed=7)
        ref = ref + r.to(D)
        kw["res"] = dev(r)
    elif epi == "muladd":
        m, a = _rnd(B, N, H, W, seed=8), _rnd(B, N, H, W, seed=9)
        ref = ref * m.to(D) + a.to(D)
        kw["muladd"] = (dev(m), dev(a))
    wd, bd = dev(w), dev(bias)

    def check(got):
        assert rel_rms(got.cpu(), ref) < 2e-6, name             # the bound of test_conv1x1_variants
        if want_stats:
            st = got._fdn_stats.cpu().view(B, 2, H, W)
            assert rel_rms(st[:, 0], ref.mean(1)) < 1e-5 and rel_rms(st[:, 1], 1 / torch.sqrt(ref.var(1, unbiased=False) + 1e-5)) < 1e-5, name

    xin_dev = xs.to(BF) if xbf else xs
    rt = ops.conv1x1(xin_dev, wd, bd, act=act, want_stats=want_stats, route_only=True, **kw)
    assert conv1x1_route_name(rt) == route, rt                  # the kernel this case is here for
    got = ops.conv1x1(xin_dev, wd, bd, act=act, want_stats=want_stats, **kw)
    check(got)
    if xbf:                                                     # storage only: the fp32 form fed the stored values, bit for bit
        f32 = ops.conv1x1(xs, wd, bd, act=act, want_stats=want_stats, **kw)
        check(f32)
        assert got.dtype == torch.float32 and torch.equal(got, f32) and torch.equal(got._fdn_stats, f32._fdn_stats)
