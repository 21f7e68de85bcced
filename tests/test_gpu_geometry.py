"""GPU: the kernels whose launch geometry follows the CU count, run under several CU budgets (fdn_hip.set_cu_budget, ABI 16) against
float64, and bit for bit against themselves.

Two families decide their geometry from fdn_device_cus():
  - persistent tile loops (grid = budget x per_cu, capped by the work; a workgroup walks tile += gridDim.x and prefetches the next tile
    while it computes the current one): every fdn_conv1x1 form reached without a weight cache, the fp32-MFMA 3x3 conv, fdn_fcaffn_in,
    fdn_fdsa_out, fdn_ffn_tail form 0;
  - channel groups per workgroup, the last one ragged and each group software-pipelined one channel ahead: fdn_fdffn_mid (CPB, 4..22),
    fdn_fdsa_core (EPB, 1..8).
At the device's own count (256 CUs) the small shapes of the other modules give every workgroup one tile and every group 4 channels; the
budgets below make the same kernels walk many tiles (crossing image boundaries: every workgroup sees tiles of both images) and reach
the channel-group clamps.  Each case is held to the float64 bound the suite already applies to that kernel, and every budget must give
the same bits as the device's count: no kernel here splits a reduction across workgroups, so which workgroup ran a pixel or a channel
must not show in it.

Persistent kernels (the conv1x1 rows: tests/common.py CONV1X1_GEOMETRY_ROUTES holds the instantiation, threads and pixel tile of each case as
fdn_conv1x1_route reports them; test_conv1x1_geometry asserts them before it runs and the CPU suite pins them): tiles per image T, pixel tile, per_cu cap of the launcher (grid = budget x per_cu <= tiles), B = 2 except where noted.
P = 84 x 131 = 11004 (P % 4 == 0: the 16-byte-lane forms) or 83 x 131 = 10873 (odd P: the scalar forms); W is never a tile multiple.

  case                     kernel (launcher)                          tile px  T/img  total  per_cu  tiles per workgroup at budget 1 / 2 / 3 / 7
  conv1x1 smallk_res       conv1x1_smallk_kernel<1, LN>               256      43     86     <= 3    >= 28 / 14 / 9 / 4
  conv1x1 smallk_vec       conv1x1_smallk_vec_kernel<1, LN, 2>        256      43     86     <= 4    >= 21 / 10 / 7 / 3
  conv1x1 smallk_muladd    conv1x1_smallk_kernel<1, LN_MULADD>        256      43     86     <= 3    >= 28 / 14 / 9 / 4
  conv1x1 smallk_stream    conv1x1_smallk_stream_kernel<3, LN>        256      43     86     1       86 / 43 / 28 / 12
  conv1x1 stream_vec       conv1x1_smallk_stream_vec_kernel<3, NONE>  512      22     44     1       44 / 22 / 14 / 6
  conv1x1 ln3_resident     conv1x1_kernel<1, LN3_GATE, 8> (resident)  256      43     86     <= 2    >= 43 / 21 / 14 / 6
  conv1x1 ln3_streaming    conv1x1_kernel<5, LN3_GATE, 4> (stream.)   128      86     172    <= 4    >= 43 / 21 / 14 / 6
  conv1x1 act_res_stats    conv1x1_kernel<4, NONE, 4> (streaming)     128      86     172    <= 4    >= 43 / 21 / 14 / 6
  conv1x1 early_muladd     conv1x1_kernel<1, LN_MULADD, 4, early>     128      85     170    <= 4    >= 42 / 21 / 14 / 6
  conv1x1 kstream_vec      conv1x1_kstream_vec_kernel<2>              256      43     86     <= 4    >= 21 / 10 / 7 / 3
  conv1x1 narrow_tail      conv1x1_smallk_vec_kernel<3, NONE, 2, TAIL> 256     43     86     <= 4    >= 21 / 10 / 7 / 3
  conv3x3 12->72, 20->100  conv3x3_kernel<3 | 4, 4>                   128      85     170    <= 4    >= 42 / 21 / 14 / 6
  fcaffn_in C=32           fcaffn_in_kernel<1, 2>  (84 x 130)         256      43     86     <= 4    >= 21 / 10 / 7 / 3
  fcaffn_in C=64           fcaffn_in_kernel<2, 1>  (84 x 130)         128      86     172    <= 4    >= 43 / 21 / 14 / 6
  fdsa_out fp32 E=38       fdsa_out_kernel<19, 1>  (odd P)            128      85     170    <= 2    >= 85 / 42 / 28 / 12
  fdsa_out vec E=38        fdsa_out_vec_kernel<19, 1, DB>             256      43     86     2       43 / 21 / 14 / 6
  fdsa_out vec E=76 bf16   fdsa_out_vec_kernel<38, 2, ., ., 1, 8, PBF> 256     43     86     1       86 / 43 / 28 / 12
  fdsa_out vec E=76 narrow fdsa_out_vec_kernel<38, 2>                 256      43     86     2       43 / 21 / 14 / 6
  ffn_tail form 0          ffn_tail_kernel<1 | 2>  (83 x 100)         8 x 32   44     88     2       44 / 22 / 14 / 6

(">=": per_cu comes from the occupancy query or an LDS quotient; the bound uses its cap.  The grids measured on an MI355X are in
profiles/r07_geometry_grids.txt.  No total above is a multiple of any grid
below 28 except 1, 2 and 43 - ragged last rounds everywhere.)

Channel groups: 32 x 64 pixel tiles, B = 2 at 64 x 96 (4 tiles per image, W not a tile multiple): groups = ceil(24 budget / (tiles x B)),
clamped; CPB_TABLE / EPB_TABLE below list (channels per group, channels of the ragged last group) per budget, and
test_channel_group_table_is_the_launch_code ties them to the launch code's formula (_cpb / _epb).
"""
import ctypes

import pytest
import torch

import fdn_oracle as O
from common import CONV1X1_GEOMETRY_ROUTES, assert_close_cond, conv1x1_route_name, rel_rms

from common import poison_uninitialized  # noqa: F401  (autouse, tests/common.py: torch.empty is filled with NaN / the integer maximum)
pytestmark = pytest.mark.gpu
F = torch.nn.functional
D = torch.float64
BUDGETS = (1, 2, 3, 7, 0)          # 0 = the device's own count (the reference geometry of the bitwise check)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import fdn_hip
    fdn_hip.lib()
    from fdn_hip import ops
    yield ops
    fdn_hip.set_cu_budget(0)


def dev(t):
    return t.to("cuda:0").contiguous()


def _rnd(*s, seed):
    return torch.randn(*s, generator=torch.Generator().manual_seed(seed))


def under_budgets(fn):
    """{budget: fn()} with every result copied to the host; the device's count is restored whatever happens."""
    import fdn_hip
    outs = {}
    try:
        for b in BUDGETS:
            fdn_hip.set_cu_budget(b)
            r = fn()
            outs[b] = tuple(t.cpu() for t in r) if isinstance(r, tuple) else r.cpu()
    finally:
        fdn_hip.set_cu_budget(0)
    return outs


def assert_invariant(outs, what):
    """every budget gives the bits of the device's count (outputs and statistics alike)"""
    ref = outs[0] if isinstance(outs[0], tuple) else (outs[0],)
    for b, r in outs.items():
        r = r if isinstance(r, tuple) else (r,)
        for i, (x, y) in enumerate(zip(r, ref)):
            assert torch.equal(x, y), f"{what}: output {i} at a budget of {b} CUs differs from the device's count " \
                                      f"(max |diff| {(x.double() - y.double()).abs().max().item():.3e})"


# ---------------------------------------------------------------------------------------------------------------------------------
# the channel-group choice of fdn_fdffn_mid / fdn_fdsa_core (csrc/patchfft.hip), restated: what the cases below are chosen for
# ---------------------------------------------------------------------------------------------------------------------------------
def _cpb(Hd, tiles, B, cus):
    groups = -(-24 * cus // (tiles * B))
    groups = min(max(groups, -(-Hd // 22)), -(-Hd // 4))
    return -(-Hd // groups)


def _epb(E, tiles, B, cus):
    groups = min(max(-(-24 * cus // (tiles * B)), 1), E)
    return min(-(-E // groups), 8)


# (channels, budget) -> (per group, last group); 256 = the MI355X's count
CPB_TABLE = {86: {1: (22, 20), 2: (15, 11), 3: (10, 6), 7: (5, 1), 256: (4, 2)},
             172: {1: (22, 18), 2: (22, 18), 3: (20, 12), 7: (9, 1), 256: (4, 4)},
             345: {1: (22, 15), 2: (22, 15), 3: (22, 15), 7: (17, 5), 256: (4, 1)},
             127: {1: (22, 17), 2: (22, 17), 3: (15, 7), 7: (7, 1), 256: (4, 3)}}
EPB_TABLE = {153: {1: (8, 1), 2: (8, 1), 3: (8, 1), 7: (8, 1), 256: (1, 1)},
             61: {1: (8, 5), 2: (8, 5), 3: (7, 5), 7: (3, 1), 256: (1, 1)}}


def _last(n, per):
    return n - (-(-n // per) - 1) * per


def test_channel_group_table_is_the_launch_code():
    for Hd, row in CPB_TABLE.items():
        for cus, (per, last) in row.items():
            c = _cpb(Hd, 4, 2, cus)
            assert (c, _last(Hd, c)) == (per, last), (Hd, cus)
    for E, row in EPB_TABLE.items():
        for cus, (per, last) in row.items():
            e = _epb(E, 4, 2, cus)
            assert (e, _last(E, e)) == (per, last), (E, cus)


def test_cu_budget_bounds(ops):
    """0 and 1 .. the device's count are accepted; the wrapper records what it set; nothing above the count is."""
    import fdn_hip
    n = torch.cuda.get_device_properties(0).multi_processor_count
    try:
        for b in (1, n):
            fdn_hip.set_cu_budget(b)
            assert fdn_hip.cu_budget() == b
        for b in (-1, n + 1):
            with pytest.raises(fdn_hip.FdnHipError):
                fdn_hip.set_cu_budget(b)
            assert fdn_hip.cu_budget() == n
    finally:
        fdn_hip.set_cu_budget(0)
    assert fdn_hip.cu_budget() == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# fdn_conv1x1, every form without a weight cache (the kernel each case reaches: CONV1X1_GEOMETRY_ROUTES, asserted below; csrc/conv1x1_route.hpp)
# ---------------------------------------------------------------------------------------------------------------------------------
CONV1X1 = {   # name: K, N, H, W, prologue, epilogue, act, want_stats, x passed as a channel slice
    "smallk_res": (32, 152, 84, 131, "ln", "res", 0, False, True),
    "smallk_vec": (32, 152, 84, 131, "ln", None, 0, False, False),
    "smallk_muladd": (32, 64, 84, 131, "muladd", "muladd", 0, False, False),
    "smallk_stream": (96, 200, 84, 131, "ln", "res", 0, False, True),
    "stream_vec": (96, 200, 84, 131, None, None, 0, False, False),
    "ln3_resident": (114, 32, 84, 131, "ln3", "res", 0, True, True),
    "ln3_streaming": (459, 160, 84, 131, "ln3", None, 0, False, True),
    "act_res_stats": (200, 100, 84, 131, None, "res", 1, True, True),
    "early_muladd": (32, 32, 83, 131, "muladd", "muladd", 0, False, False),
    "kstream_vec": (172, 64, 84, 131, None, "res", 0, True, False),
    "narrow_tail": (86, 32, 84, 131, None, "res", 0, True, False),
}


@pytest.mark.parametrize("name", list(CONV1X1))
def test_conv1x1_geometry(ops, name):
    K, N, H, W, pro, epi, act, want_stats, sliced = CONV1X1[name]
    B = 2
    x, w = _rnd(B, K, H, W, seed=1) * 1.5 + 0.3, _rnd(N, K, seed=2) / K ** 0.5
    bias = _rnd(N, seed=3) * 0.1
    # the activations as a channel slice of a wider tensor (batch stride != K * P): what ops.py allows for every conv1x1 operand
    wide = dev(torch.cat([_rnd(B, 3, H, W, seed=20), x, _rnd(B, 5, H, W, seed=21)], 1)) if sliced else None
    xs = wide[:, 3:3 + K] if sliced else dev(x)
    xd = x.to(D)
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
        full = dev(torch.cat([x, vv], 1))                       # v_value a slice as well: [o1|o2|o3|v_value] as fdsa_core leaves them
        if sliced:
            xs = full[:, :K]
        kw["ln3_gate"] = (ops.chan_stats(xs, groups=3), dev(g), dev(b_), full[:, K:])
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
    rt = ops.conv1x1(xs, wd, bd, act=act, want_stats=want_stats, route_only=True, **kw)
    assert (conv1x1_route_name(rt), rt["threads"], rt["tile_px"]) == CONV1X1_GEOMETRY_ROUTES[name], rt      # the kernel this case is here for

    def run():
        out = ops.conv1x1(xs, wd, bd, act=act, want_stats=want_stats, **kw)
        return (out, out._fdn_stats) if want_stats else out
    outs = under_budgets(run)
    for b, r in outs.items():
        got = r[0] if want_stats else r
        assert rel_rms(got, ref) < 2e-6, (name, b)             # the bound of test_conv1x1_variants
        if want_stats:
            st = r[1].view(B, 2, H, W)
            assert rel_rms(st[:, 0], ref.mean(1)) < 1e-5, (name, b)
            assert rel_rms(st[:, 1], 1 / torch.sqrt(ref.var(1, unbiased=False) + 1e-5)) < 1e-5, (name, b)
    assert_invariant(outs, f"conv1x1 {name}")


# ---------------------------------------------------------------------------------------------------------------------------------
# the fp32-MFMA 3x3 conv (csrc/conv3x3.hip conv3x3_kernel: Cin % 8 != 0 with Cout > 64; the LDS-tiled split-bf16 form's grid follows
# the work and is not CU-dependent)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cin,Cout", [(12, 72), (20, 100)])
def test_conv3x3_geometry(ops, Cin, Cout):
    B, H, W = 2, 83, 131
    x, w, bias = _rnd(B, Cin, H, W, seed=1), _rnd(Cout, Cin, 3, 3, seed=2) / (3 * Cin ** 0.5), _rnd(Cout, seed=3)
    res = _rnd(B, Cout, H, W, seed=4)
    ref = torch.relu(F.conv2d(x.to(D), w.to(D), bias.to(D), padding=1)) + res.to(D)
    xd, wd, bd, rd = dev(x), dev(w), dev(bias), dev(res)
    outs = under_budgets(lambda: ops.conv2d(xd, wd, bd, pad=1, act=2, res=rd))
    for b, got in outs.items():
        assert rel_rms(got, ref) < 2e-6, b                      # the bound of test_conv3x3_paths
    assert_invariant(outs, f"conv3x3 {Cin}->{Cout}")


# ---------------------------------------------------------------------------------------------------------------------------------
# fdn_fcaffn_in (FDN_arch.py:419-423)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,x1_ln", [(32, True), (64, False)])
def test_fcaffn_in_geometry(ops, C, x1_ln):
    B, H, W = 2, 84, 130
    xi, x1 = _rnd(B, C, H, W, seed=1) * 1.3 + 0.2, _rnd(B, C, H, W, seed=2) * 2.0 + 0.5
    img = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(3))
    w = _rnd(C, C, seed=4) / C ** 0.5
    g, b_ = _rnd(C, seed=5) * 0.2 + 1.0, _rnd(C, seed=6) * 0.1
    w1m, w3m, w1a, w3a = _rnd(C, 3, seed=7), _rnd(C, 9, seed=8) / 3, _rnd(C, 3, seed=9), _rnd(C, 9, seed=10) / 3
    g1, b1 = _rnd(C, seed=11) * 0.2 + 1.0, _rnd(C, seed=12) * 0.1
    x1n = O.ln_chan(x1.to(D), g1.to(D), b1.to(D)) if x1_ln else x1.to(D)
    u = O.ln_chan(xi.to(D), g.to(D), b_.to(D)) * x1n + x1n
    t = torch.einsum("nk,bkhw->bnhw", w.to(D), u)
    m64 = F.conv2d(F.conv2d(img.to(D), w1m.to(D).view(C, 3, 1, 1)), w3m.to(D).view(C, 1, 3, 3), padding=1, groups=C)
    a64 = F.conv2d(F.conv2d(img.to(D), w1a.to(D).view(C, 3, 1, 1)), w3a.to(D).view(C, 1, 3, 3), padding=1, groups=C)
    ref = t * m64 + a64
    a = [dev(v) for v in (xi, x1, img, w, g, b_, w1m, w3m, w1a, w3a)]
    ln1 = (ops.chan_stats(a[1]), dev(g1), dev(b1)) if x1_ln else None
    outs = under_budgets(lambda: ops.fcaffn_in(*a, x1_ln=ln1))
    for b, got in outs.items():
        assert rel_rms(got, ref) < 2e-6, b                      # the bound of test_fcaffn_in_equals_unfused
    assert_invariant(outs, f"fcaffn_in C={C}")


# ---------------------------------------------------------------------------------------------------------------------------------
# fdn_fdsa_out (FDN_arch.py:633-639, :671): three LayerNorms * v_value, project_out, residual, statistics
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,E,N,H", [("fp32", 38, 32, 83), ("vec", 38, 32, 84), ("vec", 76, 64, 84), ("vec-narrow", 76, 64, 84)])
def test_fdsa_out_geometry(ops, form, E, N, H):
    import fdn_hip
    B, W = 2, 131
    P = H * W                                                   # odd P: no 16-byte lanes, the fp32 form
    g = torch.Generator().manual_seed(11)
    o, w = torch.randn(B, 4 * E, P, generator=g), torch.randn(N, 3 * E, generator=g) / (3 * E) ** .5
    g3, b3, res = torch.randn(3 * E, generator=g), torch.randn(3 * E, generator=g), torch.randn(B, N, P, generator=g)
    od, v = o.to(D), o.to(D)[:, 3 * E:]
    parts = []
    for k in range(3):
        og = od[:, k * E:(k + 1) * E]
        mu, var = og.mean(1, keepdim=True), og.var(1, unbiased=False, keepdim=True)
        parts.append(((og - mu) / torch.sqrt(var + 1e-5) * g3[k * E:(k + 1) * E].to(D)[None, :, None] + b3[k * E:(k + 1) * E].to(D)[None, :, None]) * v)
    ref = torch.einsum("nk,bkp->bnp", w.to(D), torch.cat(parts, 1)) + res.to(D)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    od_, wd, gd, bd, rd = dev(o), dev(w), dev(g3), dev(b3), dev(res)

    def run():
        out = torch.full((B, N, P), float("nan"), device="cuda:0")
        st = torch.full((B, 2, P), float("nan"), device="cuda:0")
        assert fdn_hip.lib().fdn_fdsa_out(ptr(od_), ptr(wd), ptr(gd), ptr(bd), ptr(rd), ptr(out), ptr(st), B, E, N, P, 0, fdn_hip.stream()) == 0
        return out, st
    try:
        fdn_hip.set_matrix_pipe("bf16-narrow" if form == "vec-narrow" else "bf16")
        outs = under_budgets(run)
    finally:
        fdn_hip.set_matrix_pipe("bf16")
    for b, (out, st) in outs.items():
        assert rel_rms(out, ref) < 2e-6, b                      # the bounds of test_fdsa_out_level2_on_the_bf16_pipe
        assert rel_rms(st[:, 0], ref.mean(1)) < 1e-5 and rel_rms(st[:, 1], 1 / torch.sqrt(ref.var(1, unbiased=False) + 1e-5)) < 1e-5, b
    assert_invariant(outs, f"fdsa_out {form} E={E}")


# ---------------------------------------------------------------------------------------------------------------------------------
# fdn_ffn_tail form 0 (the persistent chunked kernel): gate + project_out + residual + statistics
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,N", [(86, 32), (45, 40)])
def test_ffn_tail_geometry(ops, C, N):
    import fdn_hip
    B, H, W = 2, 83, 100
    y, wd, w, res = _rnd(B, C, H, W, seed=1), _rnd(2 * C, 1, 3, 3, seed=2) * 0.3, _rnd(N, C, seed=3) / C ** 0.5, _rnd(B, N, H, W, seed=4)
    a, gt = F.conv2d(y.to(D), wd.to(D), padding=1, groups=C).chunk(2, 1)
    ref = F.conv2d(F.gelu(a) * gt, w.to(D).view(N, C, 1, 1)) + res.to(D)
    yd, wdd, wdv, rd = dev(y), dev(wd), dev(w), dev(res)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def run():
        out = torch.empty(B, N, H, W, device="cuda:0")
        st = torch.empty(B, 1, 2, H * W, device="cuda:0")
        assert fdn_hip.lib().fdn_ffn_tail(p(yd), p(wdd), p(wdv), p(rd), p(out), p(st), B, C, N, H, W, 0, 0, fdn_hip.stream()) == 0
        return out, st
    outs = under_budgets(run)
    for b, (out, st) in outs.items():
        assert rel_rms(out, ref) < 3e-6, b                      # the bounds of test_ffn_tail_fused_equals_reference
        st = st.view(B, 2, H, W)
        assert rel_rms(st[:, 0], ref.mean(1)) < 1e-5 and rel_rms(st[:, 1], 1 / torch.sqrt(ref.var(1, unbiased=False) + 1e-5)) < 1e-5, b
    assert_invariant(outs, f"ffn_tail C={C} N={N}")


# ---------------------------------------------------------------------------------------------------------------------------------
# fdn_fdffn_mid and fdn_fdsa_core: channel groups per workgroup (the pieces of oracle/fdn_oracle.py fdffn / fdsa, restated from their
# inputs: the float64 truth and the fp32 reference of assert_close_cond are the same restatement in two precisions)
# ---------------------------------------------------------------------------------------------------------------------------------
def _mid(x, w0, w2, fa, fp):
    """FDN_arch.py:457-470 from the project_in output (oracle fdffn between project_in and dwconv)"""
    hd = x.shape[1]
    s = F.conv2d(F.gelu(F.conv2d(x, w0, padding=1, groups=hd)), w2, padding=1, groups=hd)
    z = O.replace_denormals(torch.fft.rfft2(O.to_patches(x)))
    z = O.polar(z.abs() * fa, z.angle() - fp)
    return O.from_patches(torch.fft.irfft2(z, s=(8, 8))) + s


def _core(h, dw, fw):
    """FDN_arch.py:578-632 from the to_hidden output (oracle fdsa between to_hidden and the LayerNorms): (o1|o2|o3|v_value)"""
    q, k, v, vv = F.conv2d(h, dw, padding=1, groups=h.shape[1]).chunk(4, 1)
    qf, kf, vf = (torch.fft.rfft2(O.to_patches(t)) for t in (q, k, v))
    vf = O.replace_denormals(vf * fw)
    qka = O.replace_denormals(qf * kf).abs()
    v_a, v_p = vf.abs(), vf.angle()
    qkp = O.replace_denormals(qf).angle() - O.replace_denormals(kf).angle()
    o = [O.from_patches(torch.fft.irfft2(O.polar(a, p), s=(8, 8))) for a, p in ((v_a, qkp), (qka, v_p), (qka, qkp))]
    return torch.cat(o + [vv], 1)


@pytest.mark.parametrize("Hd,storage", [(86, "f32"), (172, "f32"), (345, "f32"), (127, "f32"), (86, "bf16"), (127, "bf16")])
def test_fdffn_mid_geometry(ops, Hd, storage):
    """fp32: against float64 with the conditioning-aware bound.  bf16 (in and out): the bf16 result is the fp32-out result of the same
    stored input rounded to nearest-even (test_bf16_is_storage_only), and that fp32-out result is held to float64 of the stored input."""
    B, H, W = 2, 64, 96
    x = _rnd(B, Hd, H, W, seed=1)
    w0, w2 = _rnd(Hd, 1, 3, 3, seed=5) / 3, _rnd(Hd, 1, 3, 3, seed=6) / 3
    fa, fp = _rnd(Hd, 1, 1, 8, 5, seed=7) * 0.2 + 1, _rnd(Hd, 1, 1, 8, 5, seed=8) * 0.5
    if storage == "bf16":
        x = x.to(torch.bfloat16).float()                        # the values the kernel reads
    truth, ref32 = _mid(x.to(D), w0.to(D), w2.to(D), fa.to(D), fp.to(D)), _mid(x, w0, w2, fa, fp)
    xd, a = dev(x), [dev(t) for t in (w0, w2, fa, fp)]
    if storage == "bf16":
        xb = xd.to(torch.bfloat16)
        outs = under_budgets(lambda: (ops.fdffn_mid(xb, *a), ops.fdffn_mid(xb, *a, out_dtype=torch.float32)))
        for b, (o16, o32) in outs.items():
            assert o16.dtype == torch.bfloat16 and torch.equal(o16, o32.to(torch.bfloat16)), b
            assert_close_cond(o32, ref32, truth, f"fdffn_mid bf16 Hd={Hd} budget {b}")
    else:
        outs = under_budgets(lambda: ops.fdffn_mid(xd, *a))
        for b, got in outs.items():
            assert_close_cond(got, ref32, truth, f"fdffn_mid Hd={Hd} budget {b}")
    assert_invariant(outs, f"fdffn_mid Hd={Hd} {storage}")


@pytest.mark.parametrize("E", [153, 61])
def test_fdsa_core_geometry(ops, E):
    B, H, W = 2, 64, 96
    h = _rnd(B, 4 * E, H, W, seed=1)
    dw, fw = _rnd(4 * E, 1, 3, 3, seed=5) / 3, _rnd(E, 1, 1, 8, 5, seed=6) * 0.2 + 1.0
    truth, ref32 = _core(h.to(D), dw.to(D), fw.to(D)), _core(h, dw, fw)
    hd, dwd, fwd = dev(h), dev(dw), dev(fw)
    outs = under_budgets(lambda: ops.fdsa_core(hd, dwd, fwd))
    for b, got in outs.items():
        assert_close_cond(got, ref32, truth, f"fdsa_core E={E} budget {b}")
    assert_invariant(outs, f"fdsa_core E={E}")
