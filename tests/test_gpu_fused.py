"""GPU parity tests of the round-2 fused kernels: each fused launch against the unfused launches it replaces
(same C ABI, same inputs) and against the CPU oracle."""
import os
import sys

import pytest
import torch

import fdn_oracle as O
from common import fdn_weights, fixture, fixture_weights, lpnet_weights, rel_rms

from common import poison_uninitialized  # noqa: F401  (autouse, tests/common.py: torch.empty is filled with NaN / the integer maximum)
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import fdn_hip
    fdn_hip.lib()   # fail loudly if the HIP extension is not built
    from basicsr.models.archs import FDN_arch
    return FDN_arch


def dev(t):
    return t.to("cuda:0").contiguous()


def _rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("C,H,W,B,ln", [(32, 32, 64, 2, True), (32, 40, 48, 1, True), (64, 16, 40, 2, True), (24, 24, 72, 2, True),
                                        (48, 8, 8, 3, True), (32, 16, 32, 1, False), (64, 368, 640, 1, True)])
def test_fdsa_fused_equals_unfused(A, C, H, W, B, ln):
    """fdn_fdsa_fused (LayerNorm + to_hidden on the bf16 matrix pipe with exactly split fp32 operands + core, one launch)
    against fdn_conv1x1 (fp32 MFMA) -> fdn_fdsa_core on the same inputs, both held to the float64 oracle: the fused launch may
    not be further from float64 than the unfused one beyond the conditioning-aware bound of the block tests."""
    from common import assert_close_cond
    from fdn_hip import ops
    E = int(C * 1.2)
    x = _rnd(B, C, H, W, seed=1) * 1.5 + 0.3
    w = _rnd(4 * E, C, seed=2) / C ** 0.5
    g, b_ = _rnd(C, seed=3) * 0.2 + 1.0, _rnd(C, seed=4) * 0.1
    dw, fw = _rnd(4 * E, 1, 3, 3, seed=5) / 3, _rnd(E, 1, 1, 8, 5, seed=6) * 0.2 + 1.0
    xd, wd, gd, bd, dwd, fwd = dev(x), dev(w), dev(g), dev(b_), dev(dw), dev(fw)
    if ln:
        st = ops.chan_stats(xd)
        hidden = ops.conv1x1(xd, wd, ln=(st, gd, bd))
        wpk = ops.fdsa_pack(wd, gd, bd)
    else:
        st = None
        hidden = ops.conv1x1(xd, wd)
        wpk = ops.fdsa_pack(wd, None, None)
    ref = ops.fdsa_core(hidden, dwd, fwd)
    got = ops.fdsa_fused(xd, st, wpk, dwd, fwd)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all()
    # float64 truth of the same front half (oracle/fdn_oracle.py fdsa, taps = the inputs of norm1/2/3 and v_value)
    D = torch.float64
    xin = O.ln_chan(x.to(D), g.to(D), b_.to(D)) if ln else x.to(D)
    P = {"a.to_hidden.weight": w.to(D).view(4 * E, C, 1, 1), "a.to_hidden_dw.weight": dw.to(D), "a.fft": fw.to(D),
         "a.project_out.weight": torch.zeros(1, 3 * E, 1, 1, dtype=D)}
    for n in ("norm1", "norm2", "norm3"):
        P[f"a.{n}.body.weight"], P[f"a.{n}.body.bias"] = torch.ones(E, dtype=D), torch.zeros(E, dtype=D)
    taps = {}
    O.fdsa(xin, P, "a", taps)
    truth = torch.cat([taps["o1"], taps["o2"], taps["o3"], taps["vv"]], 1)
    e_got, e_ref = assert_close_cond(got, ref, truth, f"fdsa_fused C={C}")
    print(f"fdsa_fused C={C} {H}x{W}: relative RMS error vs float64: fused {e_got:.2e}, unfused {e_ref:.2e}")


def test_fdsa_fused_batch_slices_and_edges(A):
    """x handed over as a batch slice of a larger tensor; partial 32-wide tiles (W = 40); zero padding at every border."""
    from fdn_hip import ops
    C, E, H, W = 32, 38, 16, 40
    big = dev(_rnd(5, C, H, W, seed=11))
    x = big[1:4]
    w = dev(_rnd(4 * E, C, seed=12) / C ** 0.5)
    g, b_ = dev(torch.ones(C)), dev(_rnd(C, seed=13))          # a bias: the out-of-image halo must still read as 0
    dw, fw = dev(_rnd(4 * E, 1, 3, 3, seed=14) / 3), dev(torch.ones(E, 1, 1, 8, 5))
    st = ops.chan_stats(x.contiguous())
    wpk = ops.fdsa_pack(w, g, b_)
    got = ops.fdsa_fused(x, st, wpk, dw, fw)
    ref = ops.fdsa_core(ops.conv1x1(x.contiguous(), w, ln=(st, g, b_)), dw, fw)
    assert rel_rms(got.cpu(), ref.cpu()) < 2e-6          # (different multipliers, fp32 both: equal to rounding, amplified by the phase arithmetic)


@pytest.mark.xfail(strict=False, reason="multi-stream runs are not bit-stable on MI355X / ROCm 7.2 beside bf16-MFMA kernels (DESIGN.md 4.7)")
def test_forward_streams_cold_start(A, monkeypatch):
    """(opt-in experiment: FDN_HIP_ALLOW_MULTISTREAM=1; the strict test of the event ordering is test_weight_cache_event_ordering)
    A freshly constructed model driven from three HIP streams at once: the derived weights (LayerNorm folds, packed
    MFMA operands, BN folds) are built on whichever stream gets there first and every other stream must wait for them
    (the first multi-stream call used to race)."""
    from basicsr.models.archs.LPNet_arch import I_predict_net
    from fdn_hip.pipeline import MULTISTREAM_ENV, forward_streams
    monkeypatch.setenv(MULTISTREAM_ENV, "1")

    def fresh():
        net = A.FDN()
        net.load_state_dict(fdn_weights(tame=0.03), strict=True)
        lp = I_predict_net()
        lp.load_state_dict(lpnet_weights(), strict=True)
        return net.to("cuda:0").eval(), lp.to("cuda:0").eval()

    x = dev(torch.rand(8, 3, 64, 96, generator=torch.Generator().manual_seed(21)))
    net, lp = fresh()
    cold = forward_streams(net, lp, x, 3)           # first call on a cold model, 3 streams (3, 2, 3 images)
    torch.cuda.synchronize()
    net2, lp2 = fresh()
    ref = forward_streams(net2, lp2, x, 1)
    torch.cuda.synchronize()
    assert torch.equal(cold, ref)


def test_weight_cache_event_ordering(A):
    """STRICT: a WeightCache entry built on one HIP stream is event-ordered before another stream reads it, without any
    kernel of this library overlapping another (the overlap is what DESIGN.md 4.7 forbids; the ordering is what a cold model driven
    from a second stream relies on).  The build enqueues a long fill in front of the value on stream A; stream B hits the entry
    at once and copies it: the copy must hold the final value."""
    from fdn_hip import ops
    c = ops.WeightCache()
    src = torch.nn.Parameter(torch.ones(4, device="cuda:0"))
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    big = torch.zeros(64 << 20, device="cuda:0")

    def build():
        for _ in range(20):
            big.add_(1.0)                       # ~ milliseconds of work queued in front of the value
        return big[:1024] * 0 + 7.0
    torch.cuda.synchronize()
    with torch.cuda.stream(sa):
        va = c.get("k", [src], build)
    with torch.cuda.stream(sb):
        vb = c.get("k", [src], build)           # same entry, other stream: must wait for A's event
        got = vb.clone()
    torch.cuda.synchronize()
    assert va is vb and bool((got == 7.0).all())
    hit = c._store["k"]
    assert sa.cuda_stream in hit[3] and sb.cuda_stream in hit[3]


@pytest.mark.parametrize("C,H,W,B", [(32, 16, 40, 2), (32, 33, 66, 1), (64, 24, 24, 2), (64, 7, 130, 1), (32, 368, 640, 1)])
def test_fcaffn_in_equals_unfused(A, C, H, W, B):
    """fdn_fcaffn_in (statistics from the register strip, modulation maps as MFMA chains on the image patch) against
    fdn_chan_stats -> fdn_img_mod_maps -> fdn_conv1x1(LN*x1+x1 prologue, *mul+add epilogue) on the same inputs.  The maps
    use folded weights (w3 * w1 rounded once), so the two differ by rounding, not bit for bit."""
    from fdn_hip import ops
    xi, x1 = dev(_rnd(B, C, H, W, seed=1) * 1.3 + 0.2), dev(_rnd(B, C, H, W, seed=2))
    img = dev(torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(3)))
    w = dev(_rnd(C, C, seed=4) / C ** 0.5)
    g, b_ = dev(_rnd(C, seed=5) * 0.2 + 1.0), dev(_rnd(C, seed=6) * 0.1)
    w1m, w3m = dev(_rnd(C, 3, seed=7)), dev(_rnd(C, 9, seed=8) / 3)
    w1a, w3a = dev(_rnd(C, 3, seed=9)), dev(_rnd(C, 9, seed=10) / 3)
    mul, add = ops.img_mod_maps(img, w1m, w3m, w1a, w3a)
    ref = ops.conv1x1(xi, w, ln_muladd=(ops.chan_stats(xi), g, b_, x1), muladd=(mul, add))
    got = ops.fcaffn_in(xi, x1, img, w, g, b_, w1m, w3m, w1a, w3a)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all()
    assert (got - ref).abs().max().item() / ref.abs().max().item() < 4e-6
    assert rel_rms(got.cpu(), ref.cpu()) < 5e-7
    # x1 given un-normalised with its LayerNorm applied on load (norm3 of the block, FDN_arch.py:675)
    g1, b1 = dev(_rnd(C, seed=11) * 0.2 + 1.0), dev(_rnd(C, seed=12) * 0.1)
    raw = dev(_rnd(B, C, H, W, seed=13) * 2.0 + 0.5)
    via_ln = ops.fcaffn_in(xi, raw, img, w, g, b_, w1m, w3m, w1a, w3a, x1_ln=(ops.chan_stats(raw), g1, b1))
    via_copy = ops.fcaffn_in(xi, ops.layernorm_chan(raw, g1, b1), img, w, g, b_, w1m, w3m, w1a, w3a)
    assert (via_ln - via_copy).abs().max().item() / via_copy.abs().max().item() < 4e-6
    # and against plain float64 math (FDN_arch.py:419-423)
    xd, x1d = xi.double().cpu(), x1.double().cpu()
    mu, var = xd.mean(1, keepdim=True), xd.var(1, keepdim=True, unbiased=False)
    u = ((xd - mu) / torch.sqrt(var + 1e-5) * g.double().cpu().view(1, -1, 1, 1) + b_.double().cpu().view(1, -1, 1, 1)) * x1d + x1d
    t = torch.einsum("nk,bkhw->bnhw", w.double().cpu(), u)
    F = torch.nn.functional
    m64 = F.conv2d(F.conv2d(img.double().cpu(), w1m.double().cpu().view(C, 3, 1, 1)), w3m.double().cpu().view(C, 1, 3, 3), padding=1, groups=C)
    a64 = F.conv2d(F.conv2d(img.double().cpu(), w1a.double().cpu().view(C, 3, 1, 1)), w3a.double().cpu().view(C, 1, 3, 3), padding=1, groups=C)
    assert rel_rms(got.cpu(), t * m64 + a64) < 2e-6


@pytest.mark.parametrize("C,H,W,B", [(128, 16, 40, 2), (96, 9, 50, 1), (160, 8, 24, 2), (128, 5, 130, 1), (128, 184, 320, 1)])
def test_fcaffn_in_packed_equals_unfused(A, C, H, W, B):
    """fdn_fcaffn_in_packed (C >= 96: the level-3 sub-block on the split-bf16 GEMM - x1's LayerNorm on load, the LN * x1 + x1 prologue, the
    image maps as MFMA chains in the epilogue) against the unfused route and against float64 math (FDN_arch.py:419-423, :675).
    Shapes: rows shorter / longer than a 128-pixel tile (tiles crossing row ends and image borders), a 96-wide layer (FDN_lolv1),
    160 channels (a second, partial channel tile), the bench shape."""
    from fdn_hip import ops
    xi, x1 = dev(_rnd(B, C, H, W, seed=1) * 1.3 + 0.2), dev(_rnd(B, C, H, W, seed=2))
    img = dev(torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(3)))
    w = dev(_rnd(C, C, seed=4) / C ** 0.5)
    g, b_ = dev(_rnd(C, seed=5) * 0.2 + 1.0), dev(_rnd(C, seed=6) * 0.1)
    w1m, w3m = dev(_rnd(C, 3, seed=7)), dev(_rnd(C, 9, seed=8) / 3)
    w1a, w3a = dev(_rnd(C, 3, seed=9)), dev(_rnd(C, 9, seed=10) / 3)
    wpk = ops.fcaffn_in_pack(w, w1m, w3m, w1a, w3a)
    st = ops.chan_stats(xi)
    mul, add = ops.img_mod_maps(img, w1m, w3m, w1a, w3a)
    ref = ops.conv1x1(xi, w, ln_muladd=(st, g, b_, x1), muladd=(mul, add))
    got = ops.fcaffn_in_packed(xi, st, x1, img, wpk, g, b_)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all()
    assert (got - ref).abs().max().item() / ref.abs().max().item() < 4e-6
    assert rel_rms(got.cpu(), ref.cpu()) < 5e-7
    g1, b1 = dev(_rnd(C, seed=11) * 0.2 + 1.0), dev(_rnd(C, seed=12) * 0.1)
    raw = dev(_rnd(B, C, H, W, seed=13) * 2.0 + 0.5)
    own = ops.fcaffn_in_packed(xi, None, x1, img, wpk, g, b_)                  # (round 5) the kernel takes the statistics of xi itself
    assert (own - got).abs().max().item() <= 2e-6 * max(1.0, got.abs().max().item())
    via_ln = ops.fcaffn_in_packed(xi, st, raw, img, wpk, g, b_, x1_ln=(ops.chan_stats(raw), g1, b1))
    via_copy = ops.fcaffn_in_packed(xi, st, ops.layernorm_chan(raw, g1, b1), img, wpk, g, b_)
    assert (via_ln - via_copy).abs().max().item() / via_copy.abs().max().item() < 4e-6
    xd, x1d = xi.double().cpu(), x1.double().cpu()
    mu, var = xd.mean(1, keepdim=True), xd.var(1, keepdim=True, unbiased=False)
    u = ((xd - mu) / torch.sqrt(var + 1e-5) * g.double().cpu().view(1, -1, 1, 1) + b_.double().cpu().view(1, -1, 1, 1)) * x1d + x1d
    t = torch.einsum("nk,bkhw->bnhw", w.double().cpu(), u)
    F = torch.nn.functional
    m64 = F.conv2d(F.conv2d(img.double().cpu(), w1m.double().cpu().view(C, 3, 1, 1)), w3m.double().cpu().view(C, 1, 3, 3), padding=1, groups=C)
    a64 = F.conv2d(F.conv2d(img.double().cpu(), w1a.double().cpu().view(C, 3, 1, 1)), w3a.double().cpu().view(C, 1, 3, 3), padding=1, groups=C)
    assert rel_rms(got.cpu(), t * m64 + a64) < 2e-6
    import fdn_hip
    with pytest.raises(fdn_hip.FdnHipError):                     # narrow layers belong to fdn_fcaffn_in
        ops.fcaffn_in_packed(xi[:, :64].contiguous(), st, x1[:, :64].contiguous(), img, wpk, g[:64].contiguous(), b_[:64].contiguous())


def test_fcaffn_in_beyond_4m_pixels(A):
    """More than 2^22 pixels per image: the pixel -> (row, column) split of the image-patch borders leaves the exact
    float-reciprocal range and takes the integer division."""
    from fdn_hip import ops
    C, H, W, B = 32, 2052, 2048, 1
    xi, x1 = dev(_rnd(B, C, H, W, seed=1)), dev(_rnd(B, C, H, W, seed=2))
    img = dev(torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(3)))
    w = dev(_rnd(C, C, seed=4) / C ** 0.5)
    g, b_ = dev(_rnd(C, seed=5) * 0.2 + 1.0), dev(_rnd(C, seed=6) * 0.1)
    w1m, w3m = dev(_rnd(C, 3, seed=7)), dev(_rnd(C, 9, seed=8) / 3)
    w1a, w3a = dev(_rnd(C, 3, seed=9)), dev(_rnd(C, 9, seed=10) / 3)
    mul, add = ops.img_mod_maps(img, w1m, w3m, w1a, w3a)
    ref = ops.conv1x1(xi, w, ln_muladd=(ops.chan_stats(xi), g, b_, x1), muladd=(mul, add))
    got = ops.fcaffn_in(xi, x1, img, w, g, b_, w1m, w3m, w1a, w3a)
    torch.cuda.synchronize()
    # rows 2046..2051 lie past pixel 2^22: compare there and at the image borders of those rows
    assert (got[..., 2040:, :] - ref[..., 2040:, :]).abs().max().item() / ref.abs().max().item() < 4e-6
    assert (got[..., :8, :] - ref[..., :8, :]).abs().max().item() / ref.abs().max().item() < 4e-6
