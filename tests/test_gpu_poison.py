"""GPU: poisoned uninitialised memory (tests/common.py poisoned(); DESIGN.md, testing).

The wrappers allocate outputs and workspace with torch.empty, and torch's caching allocator hands a freed block to the next request of its
size: without the poison the second of two equal calls finds the first one's answer in its output, and workspace that is read before it is
written holds finite garbage.  Every tests/test_gpu_*.py runs under the module fixture common.poison_uninitialized; this module
  - establishes the premise on the device (the fill reaches device allocations, torch.zeros is untouched, the switch restores),
  - shows that the poison has teeth without touching a kernel: a destination that is a strict part of a larger poisoned allocation comes
    back finite and within the entry point's float64 bound, and every element outside it is still NaN (all inside one allocation),
  - checks the contracts that only poison can check (the padded bins of a spectrum, the padding records of the packed guidance, the
    statistics of a ragged pixel count),
  - keeps "the same call twice under different CU budgets" (test_gpu_geometry.under_budgets) in miniature as the named regression.

Two cases differ from their first statement because the library refuses the stated shape: the smallk_vec route of fdn_conv1x1 needs
P % 4 == 0 (csrc/conv1x1_route.hpp vec_aligned), so it runs at 12 x 22 (264 pixels, a 256-pixel tile and a ragged one of 8, as
test_gpu_kernel_forms.py places the pixel-pair forms) and the same shape runs at the odd 13 x 21 as well, where it takes the dword
small-K kernel; fdn_rfft_rows_ln has planned widths only (W = 40 is refused, asserted below), so it runs at 280 (Wf = 141, pitch 144)."""
import math

import pytest
import torch

import fdn_oracle as O
import lpips_ref as R
from common import CONV1X1_GEOMETRY_ROUTES, assert_close_cond, conv1x1_route_name, poisoned, poisoned_off, rel_rms
from test_gpu_geometry import _mid

from common import poison_uninitialized  # noqa: F401  (autouse, tests/common.py: torch.empty is filled with NaN / the integer maximum)
pytestmark = pytest.mark.gpu
F = torch.nn.functional
D = torch.float64
DEV = "cuda:0"
FLOATS = (torch.float32, torch.float64, torch.bfloat16)
INTS = (torch.uint8, torch.int64)


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
    return t.to(DEV).contiguous()


def _rnd(*s, seed):
    return torch.randn(*s, generator=torch.Generator().manual_seed(seed))


def _allocations(dtype):
    base = torch.zeros(3, 5, device=DEV, dtype=dtype)
    return {"empty": torch.empty(37, 5, device=DEV, dtype=dtype), "empty_like": torch.empty_like(base), "new_empty": base.new_empty((7, 3)),
            "empty_strided": torch.empty_strided((3, 5), (5, 1), device=DEV, dtype=dtype)}


# ---------------------------------------------------------------------------------------------------------------------------------
# the premise: the fill reaches device allocations
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", FLOATS + INTS, ids=lambda d: str(d).split(".")[-1])
def test_device_allocations_are_poisoned(ops, dtype):
    with poisoned():
        for how, t in _allocations(dtype).items():
            assert t.is_cuda and t.numel() > 0
            if dtype in FLOATS:
                assert bool(torch.isnan(t).all()), f"{how} {dtype}: not all-NaN"
            else:
                assert bool((t == torch.iinfo(dtype).max).all()), f"{how} {dtype}: not the type's maximum"
        z = torch.zeros(37, 5, device=DEV, dtype=dtype)
        assert bool((z == 0).all()), f"torch.zeros {dtype}"


def test_the_block_a_freed_result_leaves_is_what_the_next_call_gets(ops):
    """The hole and the switch in one place.  Without the poison (poisoned_off: listed in common.POISON_EXEMPT) a torch.empty of the size
    just freed gets that block with the old contents; under poisoned() the same request is all-NaN; after the block it is no longer forced."""
    n = 1 << 20

    def freed_then_empty():
        t = torch.full((n,), 3.0, device=DEV)
        p = t.data_ptr()
        torch.cuda.synchronize()
        del t
        u = torch.empty(n, device=DEV)
        assert u.data_ptr() == p, "the caching allocator did not hand the freed block back"
        return u

    with poisoned_off():
        assert not torch.are_deterministic_algorithms_enabled() and not torch.utils.deterministic.fill_uninitialized_memory
        assert bool((freed_then_empty() == 3.0).all())
        with poisoned():
            assert bool(torch.isnan(freed_then_empty()).all())
        assert not torch.are_deterministic_algorithms_enabled() and not torch.utils.deterministic.fill_uninitialized_memory
        assert bool((freed_then_empty() == 3.0).all())
    assert torch.are_deterministic_algorithms_enabled() and torch.is_deterministic_algorithms_warn_only_enabled()
    assert torch.utils.deterministic.fill_uninitialized_memory                      # the module fixture's state is back
    assert bool(torch.isnan(freed_then_empty()).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# teeth: a destination inside a larger poisoned allocation
# ---------------------------------------------------------------------------------------------------------------------------------
CONV1X1_PART = {   # name: K, N, H, W, prologue, the route with out = big[:, :N]
    "generic": (64, 96, 13, 21, "ln", "generic<3,ln,4,0>"),               # "ln_3" of test_gpu_kernel_forms.CONV1X1
    "smallk_vec": (32, 64, 12, 22, "ln", "smallk_vec<1,ln,obf=0>"),       # P % 4 == 0: the 8-byte-lane form
    "smallk_odd": (32, 64, 13, 21, "ln", "smallk<1,ln>"),                 # the same shape at odd P: the dword form
}


@pytest.mark.parametrize("name", list(CONV1X1_PART))
def test_conv1x1_into_part_of_a_poisoned_buffer(ops, name):
    K, N, H, W, pro, route = CONV1X1_PART[name]
    B = 2
    x, w, bias = _rnd(B, K, H, W, seed=1) * 1.5 + 0.3, _rnd(N, K, seed=2) / K ** 0.5, _rnd(N, seed=3) * 0.1
    g, b_ = _rnd(K, seed=4), _rnd(K, seed=5)
    ref = F.conv2d(O.ln_chan(x.to(D), g.to(D), b_.to(D)), w.to(D).view(N, K, 1, 1), bias.to(D))
    xd = dev(x)
    kw = dict(ln=(ops.chan_stats(xd), dev(g), dev(b_)))
    big = torch.empty(B, N + 3, H, W, device=DEV)
    assert bool(torch.isnan(big).all())
    rt = ops.conv1x1(xd, dev(w), dev(bias), out=big[:, :N], route_only=True, **kw)
    assert conv1x1_route_name(rt) == route, rt
    out = ops.conv1x1(xd, dev(w), dev(bias), out=big[:, :N], **kw)
    torch.cuda.synchronize()
    assert out.data_ptr() == big.data_ptr()
    got = big.cpu()
    assert bool(torch.isfinite(got[:, :N]).all())
    assert rel_rms(got[:, :N], ref) < 2e-6                        # the bound of test_conv1x1_variants
    assert bool(torch.isnan(got[:, N:]).all()), "planes N .. N+2 of an image were written"


@pytest.mark.parametrize("W", [26, 280])                        # a generic width (8 rows per workgroup) and a planned one; 18 rows: ragged
def test_irfft_rows_into_the_head_of_a_taller_buffer(ops, W):
    B, C, H, Wf = 2, 1, 9, W // 2 + 1
    z = _rnd(B, C, H, Wf, 2, seed=W)
    scale = 2.0 / (H * W)
    truth = torch.fft.irfft(torch.view_as_complex(z).to(torch.complex128), n=W, dim=-1) * (W / 2) * scale
    rows = B * C * H
    tall = torch.empty(rows + 5, W, device=DEV)
    out = ops.irfft_rows(dev(z), H, W, scale, out=tall[:rows].view(B, C, H, W))
    torch.cuda.synchronize()
    assert out.data_ptr() == tall.data_ptr()
    got = tall.cpu()
    assert bool(torch.isfinite(got[:rows]).all())
    assert rel_rms(got[:rows].view(B, C, H, W), truth) < 3e-6     # the bound of test_irfft_rows
    assert bool(torch.isnan(got[rows:]).all()), "rows past B * C * H were written"


@pytest.mark.parametrize("normalize", [True, False])
def test_lpips_prep_into_the_first_half(ops, normalize):
    """as LPIPS.__call__ uses it: one buffer of 2B images, in0 goes to the first B"""
    from fdn_hip import lpips
    B = 2
    x = R.images(B, 29, 41, seed=3)
    if not normalize:
        x = x * 2 - 1
    buf = torch.empty(2 * B, 3, 29, 41, device=DEV)
    lpips.prep_f32(dev(x), normalize=normalize, out=buf[:B])
    torch.cuda.synchronize()
    got = buf.cpu()
    assert torch.equal(got[:B], R.scaling(x, normalize=normalize))      # bit for bit, as test_prep_f32_bit_exact
    assert bool(torch.isnan(got[B:]).all()), "the second half was written"


def test_lpips_layer_accumulates_into_three_of_five_slots(ops):
    from fdn_hip import lpips
    B, C, H, W = 3, 64, 37, 53
    g = torch.Generator().manual_seed(C + H)
    f0, f1 = torch.relu(torch.randn(B, C, H, W, generator=g)), torch.relu(torch.randn(B, C, H, W, generator=g))
    w = torch.rand(C, generator=g)
    want = R.head(f0.double(), f1.double(), w.double()) + 0.25
    acc = torch.empty(5, dtype=D, device=DEV)
    acc[:B] = 0.25                                               # what the earlier heads left; slots 3 and 4 stay poisoned
    lpips.layer(dev(torch.cat([f0, f1])), dev(w), out=acc[:B], accumulate=True)
    torch.cuda.synchronize()
    got = acc.cpu()
    assert bool(torch.isfinite(got[:B]).all())
    assert ((got[:B] - want).abs() / want.abs()).max().item() <= 1e-10     # LAYER_RTOL of test_gpu_lpips.py
    assert bool(torch.isnan(got[B:]).all()), "a slot past B was written"


# ---------------------------------------------------------------------------------------------------------------------------------
# contracts that only poison can check
# ---------------------------------------------------------------------------------------------------------------------------------
def test_rfft_rows_padded_bins_are_zero(ops):
    """ops.rfft_rows: "bins past W//2 are zeros" - the column pass runs over the padded width"""
    W, Wf = 40, 21
    pitch = ops.spec_pitch(Wf)
    assert pitch == 32
    x = _rnd(2, 3, 9, W, seed=1)
    z = ops.rfft_rows(dev(x), pitch=pitch).cpu()
    assert z.shape == (2, 3, 9, pitch, 2)
    assert bool((z[..., Wf:, :] == 0).all()), "bins Wf .. pitch-1 are not exactly zero"
    assert rel_rms(z[..., :Wf, :], torch.view_as_real(torch.fft.rfft(x.double(), dim=-1))) < 2e-6      # the bound of test_rfft_rows


def test_rfft_rows_ln_padded_bins_are_zero(ops):
    import fdn_hip
    B, C, H = 2, 8, 9
    gm, bt = _rnd(C, seed=2) * 0.3 + 1.0, _rnd(C, seed=3) * 0.2
    x40 = dev(_rnd(B, C, H, 40, seed=1))
    with pytest.raises(fdn_hip.FdnHipError):                     # planned widths only: 40 has no form
        ops.rfft_rows_ln(x40, ops.chan_stats(x40), dev(gm), dev(bt), pitch=32)
    W, Wf = 280, 141
    pitch = ops.spec_pitch(Wf)
    assert pitch == 144 and ops.fft_route(ops.FFT_ROWS, W)["route"] == "planned"
    x = _rnd(B, C, H, W, seed=4) * 1.7 + 0.4
    xd = dev(x)
    z = ops.rfft_rows_ln(xd, ops.chan_stats(xd), dev(gm), dev(bt), pitch=pitch).cpu()
    assert z.shape == (B, C, H, pitch, 2)
    assert bool((z[..., Wf:, :] == 0).all()), "rfft_rows_ln: bins Wf .. pitch-1 are not exactly zero"
    truth = torch.view_as_real(torch.fft.rfft(O.ln_chan(x.to(D), gm.to(D), bt.to(D)), dim=-1))
    assert rel_rms(z[..., :Wf, :], truth) < 3e-6                  # the bound of test_rfft_rows_ln_equals_layernorm_then_rfft
    z = ops.rfft_rows(xd, pitch=pitch).cpu()                     # the planned kernel without the LayerNorm
    assert bool((z[..., Wf:, :] == 0).all()), "rfft_rows: bins Wf .. pitch-1 are not exactly zero"
    assert rel_rms(z[..., :Wf, :], torch.view_as_real(torch.fft.rfft(x.double(), dim=-1))) < 2e-6


def test_pack_guidance_padding_records_are_zero(ops):
    """csrc/fft2d.hip pack_guidance_kernel: a record is (amp0, amp1, amp2, pha0, pha1, pha2, 0, 0); the records w >= Wf of a padded row are
    eight zeros - amplitude 0, phase 0.  fdn_fft_cols_fcaffn runs over the padded width and multiplies the padded (zero) bins of the
    spectrum by A = wxa . amp = 0 and a rotation by 0: it must meet finite numbers there, and zeros keep the padding of z zero."""
    B, H, Wf = 2, 5, 21
    pitch = ops.spec_pitch(Wf)
    amp = _rnd(B, 3, H, Wf, seed=1).abs()
    pha = (torch.rand(B, 3, H, Wf, generator=torch.Generator().manual_seed(2)) * 2 - 1) * math.pi
    rec = ops.pack_guidance(dev(amp), dev(pha), pitch=pitch).cpu()
    assert rec.shape == (B, H, pitch, 8)
    assert bool((rec[:, :, Wf:] == 0).all()), "a padding record is not eight zeros"
    assert torch.equal(rec[:, :, :Wf, 0:3], amp.permute(0, 2, 3, 1)) and torch.equal(rec[:, :, :Wf, 3:6], pha.permute(0, 2, 3, 1))
    assert bool((rec[:, :, :Wf, 6:] == 0).all()), "the two spare floats of a record are not zero"


@pytest.mark.parametrize("C,groups", [(12, 1), (114, 3)])
def test_chan_stats_ragged_pixel_count(ops, C, groups):
    """P = 13 x 21 = 273: one 256-pixel round and a ragged one; every one of the 2 P statistics of a group is written"""
    B, H, W = 2, 13, 21
    x = _rnd(B, C, H, W, seed=C)
    st = ops.chan_stats(dev(x), groups=groups).cpu()
    assert st.shape == (B, groups, 2, H * W) and bool(torch.isfinite(st).all())
    xg = x.to(D).view(B, groups, C // groups, H * W)
    assert rel_rms(st[:, :, 0], xg.mean(2)) < 1e-5 and rel_rms(st[:, :, 1], 1 / torch.sqrt(xg.var(2, unbiased=False) + 1e-5)) < 1e-5


# ---------------------------------------------------------------------------------------------------------------------------------
# the same call twice: budget 1, free the result, then 7 and the device's count
# ---------------------------------------------------------------------------------------------------------------------------------
def _twice(fn):
    """[fn() at a budget of 1, 7 and 0 CUs], each result copied to the host and freed before the next call"""
    import fdn_hip
    outs = []
    try:
        for b in (1, 7, 0):
            fdn_hip.set_cu_budget(b)
            r = fn()
            outs.append(r.cpu())
            del r
    finally:
        fdn_hip.set_cu_budget(0)
    return outs


def test_persistent_conv1x1_same_call_at_three_budgets(ops):
    """conv1x1 smallk_res of test_gpu_geometry.CONV1X1 at 83 x 131 (odd P: 43 tiles per image, the last one ragged)"""
    K, N, H, W, B = 32, 152, 83, 131, 2
    x, w, bias = _rnd(B, K, H, W, seed=1) * 1.5 + 0.3, _rnd(N, K, seed=2) / K ** 0.5, _rnd(N, seed=3) * 0.1
    g, b_, r = _rnd(K, seed=4), _rnd(K, seed=5), _rnd(B, N, H, W, seed=7)
    ref = F.conv2d(O.ln_chan(x.to(D), g.to(D), b_.to(D)), w.to(D).view(N, K, 1, 1), bias.to(D)) + r.to(D)
    xd, wd, bd, rd = dev(x), dev(w), dev(bias), dev(r)
    kw = dict(ln=(ops.chan_stats(xd), dev(g), dev(b_)), res=rd)
    rt = ops.conv1x1(xd, wd, bd, route_only=True, **kw)
    assert (conv1x1_route_name(rt), rt["threads"], rt["tile_px"]) == CONV1X1_GEOMETRY_ROUTES["smallk_res"], rt
    outs = _twice(lambda: ops.conv1x1(xd, wd, bd, **kw))
    assert rel_rms(outs[0], ref) < 2e-6                           # the bound of test_conv1x1_variants
    for b, got in zip((1, 7, 0), outs):
        assert bool(torch.isfinite(got).all()), f"budget {b}: an element was never written"
        assert torch.equal(got, outs[0]), f"budget {b} differs from budget 1"


def test_channel_group_fdffn_mid_same_call_at_three_budgets(ops):
    """fdffn_mid Hd = 86 at 64 x 96: 22 / 5 / 4 channels per group, the last group ragged (test_gpu_geometry.CPB_TABLE)"""
    B, Hd, H, W = 2, 86, 64, 96
    x = _rnd(B, Hd, H, W, seed=1)
    w0, w2 = _rnd(Hd, 1, 3, 3, seed=5) / 3, _rnd(Hd, 1, 3, 3, seed=6) / 3
    fa, fp = _rnd(Hd, 1, 1, 8, 5, seed=7) * 0.2 + 1, _rnd(Hd, 1, 1, 8, 5, seed=8) * 0.5
    truth, ref32 = _mid(x.to(D), w0.to(D), w2.to(D), fa.to(D), fp.to(D)), _mid(x, w0, w2, fa, fp)
    xd, a = dev(x), [dev(t) for t in (w0, w2, fa, fp)]
    outs = _twice(lambda: ops.fdffn_mid(xd, *a))
    assert_close_cond(outs[0], ref32, truth, "fdffn_mid Hd=86 budget 1")
    for b, got in zip((1, 7, 0), outs):
        assert bool(torch.isfinite(got).all()), f"budget {b}: an element was never written"
        assert torch.equal(got, outs[0]), f"budget {b} differs from budget 1"
