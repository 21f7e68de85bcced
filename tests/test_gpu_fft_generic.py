"""GPU tests of the generic full-image FFT kernels (every length without a compile-time plan) against torch.fft in float64, one length
per route the host picks: in-place and ping-pong column passes at every BIG tier and tc, the gather pass at several primes, Rader rows with
plain and BIG sub-plans, generic and gather rows, the tiny and the largest lengths, and the refusals.  Each case first checks that
fdn_fft_route still sends its length down the route it is named for (tests/common.py FFT_COL_ROUTES / FFT_ROW_ROUTES).

Accuracy, per line - every column of every plane, every row - and not only per tensor, so that one wrong column tile
or row block cannot hide in an RMS: rel-RMS err(HIP, fp64) <= 4 * err(torch.fft in float32, fp64) + 2e-6.  Phases are compared through the
complex value polar(mag, ang)."""
import ctypes
import math

import pytest
import torch

from common import FFT_COL_ROUTES, FFT_ROW_ROUTES, fcaffn_ref, rel_rms

from common import poison_uninitialized  # noqa: F401  (autouse, tests/common.py: torch.empty is filled with NaN / the integer maximum)
pytestmark = pytest.mark.gpu

COLS = sorted(H for H, r in FFT_COL_ROUTES.items() if r[0] != "refused")
ROWS = sorted(W for W, r in FFT_ROW_ROUTES.items() if r[0] != "refused")
WORST = {}                # route -> worst per-line error seen (printed at the end of the module)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import fdn_hip
    fdn_hip.lib()
    from fdn_hip import ops as o
    yield o
    for k in sorted(WORST):
        print(f"worst per-line rel-RMS error  {k:34s} {WORST[k]:.2e}")


def dev(t):
    return t.to("cuda:0").contiguous()


def _rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _col_route(ops, H):
    route, big, tc, gather = FFT_COL_ROUTES[H]
    rt = ops.fft_route(ops.FFT_COLS, H)
    assert (rt["route"], rt["big"], rt["width"], rt["gather"]) == (route, big, tc, gather), (H, rt)
    return f"cols {route} BIG {big} tc {tc}" + (f" gather {gather}" if gather else "")


def _row_route(ops, W, inverse=False):
    route, big, rpb, gather, p = FFT_ROW_ROUTES[W]
    rt = ops.fft_route(ops.FFT_IROWS if inverse else ops.FFT_ROWS, W)
    if inverse:
        assert rt["route"] == "pingpong" and rt["width"] == rpb and rt["gather"] == ((p,) if p else gather), (W, rt)
        return f"irows BIG {rt['big']}" + (f" gather {rt['gather']}" if rt["gather"] else "")
    assert (rt["route"], rt["big"], rt["width"], rt["gather"], rt["rader"]) == (route, big, rpb, gather, p), (W, rt)
    return f"rows {route} BIG {big}" + (f" gather {gather}" if gather else "") + (f" p {p}" if p else "")


def _per_line(got, ref32, truth, dims, what):
    """rel-RMS error of every line (the reduction `dims` span one line): err(got) <= 4 err(fp32 torch) + 2e-6 on each."""
    got, ref32, truth = got.double().cpu(), ref32.double().cpu(), truth.double().cpu()
    norm = (truth ** 2).sum(dims).sqrt() + 1e-300
    e_got = ((got - truth) ** 2).sum(dims).sqrt() / norm
    e_ref = ((ref32 - truth) ** 2).sum(dims).sqrt() / norm
    bad = e_got > 4 * e_ref + 2e-6
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} lines, worst {e_got.max().item():.3e} (fp32 torch {e_ref.max().item():.3e})"
    WORST[what] = max(WORST.get(what, 0.0), e_got.max().item())
    return e_got.max().item()


def _tile_shape(H):
    """Wf with a ragged last column tile, and planes such that the tile total is not a multiple of 8"""
    tc = FFT_COL_ROUTES[H][2]
    return 2 * tc + 3, 3                                   # 3 tiles per plane, 9 tiles


# ---------------------------------------------------------------- columns
@pytest.mark.parametrize("H", COLS)
def test_cols_fwd(ops, H):
    what = _col_route(ops, H)
    Wf, planes = _tile_shape(H)
    z = _rnd(1, planes, H, Wf, 2, seed=H)
    mag, ang = ops.fft_cols_fwd(dev(z), True, True, rd_before=False, fix_real=False)
    truth = torch.fft.fft(torch.view_as_complex(z.double()), dim=2)
    ref32 = torch.fft.fft(torch.view_as_complex(z), dim=2)
    got = torch.polar(mag.cpu().double(), ang.cpu().double())
    _per_line(torch.view_as_real(got), torch.view_as_real(ref32), torch.view_as_real(truth), (2, 4), what)
    _per_line(mag, ref32.abs(), truth.abs(), (2,), what + " |z|")
    assert rel_rms(mag.cpu(), truth.abs()) < 2e-6
    assert rel_rms(torch.view_as_real(got), torch.view_as_real(truth)) < 3e-6
    # rd_before changes nothing on data without components in (-1e-10, 1e-10); fix_real changes only the self-conjugate bins, to Im = +0
    mag2, ang2 = ops.fft_cols_fwd(dev(z), True, True, rd_before=True, fix_real=False)
    assert torch.equal(mag2, mag) and torch.equal(ang2, ang)
    mag2, ang2 = ops.fft_cols_fwd(dev(z), True, True, rd_before=False, fix_real=True)
    keep = torch.ones(H, Wf, dtype=torch.bool)
    for h in ([0, H // 2] if H % 2 == 0 else [0]):
        keep[h, 0] = keep[h, Wf - 1] = False
    mag2, ang2 = mag2.cpu(), ang2.cpu()
    assert torch.equal(mag2[..., keep], mag.cpu()[..., keep]) and torch.equal(ang2[..., keep], ang.cpu()[..., keep])
    a = ang2[..., ~keep]
    assert ((a == 0) & ~torch.signbit(a) | (a == torch.tensor(math.pi, dtype=torch.float32))).all(), a


@pytest.mark.parametrize("H", COLS)
def test_cols_fwd_fix_real_and_denormals(ops, H):
    """fix_real on the spectrum of a real image: Im = +0 and angle = +pi exactly at the negative real self-conjugate bins (two of them at
    an odd H, four at an even H); rd_before on zeros gives |z| = sqrt(2) 1e-10, angle pi/4 everywhere."""
    _col_route(ops, H)
    W = 12
    h = torch.arange(H, dtype=torch.float64).view(-1, 1) % 2 * 2 - 1          # (-1)^(h+1)
    w = torch.arange(W, dtype=torch.float64).view(1, -1) % 2 * 2 - 1
    x = -4.0 + 0.5 * h + 0.5 * w - 0.25 * h * w + 0.01 * _rnd(H, W, seed=H).double()
    z = torch.view_as_real(torch.fft.rfft(x, dim=-1)).float().view(1, 1, H, W // 2 + 1, 2)
    truth = torch.fft.fft(torch.fft.rfft(x, dim=-1), dim=0)
    mag, ang = ops.fft_cols_fwd(dev(z), True, True, rd_before=False, fix_real=True)
    rows = [0, H // 2] if H % 2 == 0 else [0]
    pi32 = torch.tensor(math.pi, dtype=torch.float32)
    for r in rows:
        for c in (0, W // 2):
            assert truth[r, c].real < 0, (r, c)
            assert ang[0, 0, r, c].item() == pi32.item(), (H, r, c, ang[0, 0, r, c].item())
            assert abs(mag[0, 0, r, c].item() - abs(truth[r, c].item())) <= 1e-5 * abs(truth[r, c].item())
    zero = torch.zeros(1, 1, H, 3, 2)
    mag, ang = ops.fft_cols_fwd(dev(zero), True, True, rd_before=True, fix_real=False)
    assert torch.allclose(mag.cpu(), torch.full_like(mag.cpu(), 2 ** 0.5 * 1e-10), rtol=1e-6)
    assert torch.allclose(ang.cpu(), torch.full_like(ang.cpu(), math.pi / 4), rtol=1e-6)


@pytest.mark.parametrize("H", COLS)
def test_cols_inv_polar(ops, H):
    what = _col_route(ops, H) + " inv"
    Wf, planes = _tile_shape(H)
    Hin, Wfin = H + 2, Wf + 4                              # leading (H, Wf) slice of wider planes: fourier_fuse's crop
    mag = _rnd(1, planes, Hin, Wfin, seed=H).abs() + 0.1
    pha = (torch.rand(1, planes, Hin, Wfin, generator=torch.Generator().manual_seed(H + 1)) * 2 - 1) * math.pi
    z = ops.fft_cols_inv_polar(dev(mag), dev(pha), H, Wf)
    truth = torch.fft.ifft(torch.polar(mag[:, :, :H, :Wf].double(), pha[:, :, :H, :Wf].double()), dim=2) * H
    ref32 = torch.fft.ifft(torch.polar(mag[:, :, :H, :Wf], pha[:, :, :H, :Wf]), dim=2) * H
    _per_line(z, torch.view_as_real(ref32), torch.view_as_real(truth), (2, 4), what)
    assert rel_rms(z.cpu(), torch.view_as_real(truth)) < 3e-6


@pytest.mark.parametrize("H", COLS)
def test_cols_fcaffn(ops, H):
    what = _col_route(ops, H) + " fcaffn"
    Wf, _ = _tile_shape(H)
    B, C = 2, 3                                            # the guidance is indexed per batch item; 18 tiles
    z = _rnd(B, C, H, Wf, 2, seed=H)
    amp = _rnd(B, 3, H, Wf, seed=H + 1).abs()
    pha = (torch.rand(B, 3, H, Wf, generator=torch.Generator().manual_seed(H + 2)) * 2 - 1) * math.pi
    wxa, wxp = _rnd(C, 3, seed=H + 3), _rnd(C, 3, seed=H + 4)
    got = ops.fft_cols_fcaffn(dev(z).clone(), dev(amp), dev(pha), dev(wxa), dev(wxp))
    truth = fcaffn_ref(z, amp, pha, wxa, wxp)
    _per_line(got, fcaffn_ref(z, amp, pha, wxa, wxp, torch.float32), truth, (2, 4), what)
    assert rel_rms(got.cpu(), truth) < 5e-6


# ---------------------------------------------------------------- rows
def _row_counts(W):
    rpb = FFT_ROW_ROUTES[W][2]
    return sorted({1, rpb + 1, 13} | ({rpb - 1} if rpb > 1 else set()))


@pytest.mark.parametrize("W", ROWS)
def test_rfft_rows(ops, W):
    what = _row_route(ops, W)
    Wf = W // 2 + 1
    pitch = Wf + 5
    for rows in _row_counts(W):
        x = _rnd(1, 1, rows, W, seed=W + rows)
        z = ops.rfft_rows(dev(x), pitch=pitch)
        zc = z.cpu()[..., :Wf, :]
        assert zc.shape[-2] == Wf and z[..., Wf:, :].abs().max().item() == 0.0 and (z[..., Wf:, :] == 0).all()
        truth = torch.view_as_real(torch.fft.rfft(x.double(), dim=-1))
        _per_line(zc, torch.view_as_real(torch.fft.rfft(x, dim=-1)), truth, (3, 4), what)
        assert rel_rms(zc, truth) < 2e-6
        assert zc[..., 0, 1].abs().max().item() == 0.0 and zc[..., W // 2, 1].abs().max().item() == 0.0     # DC / Nyquist exactly real
        back = ops.irfft_rows(z, rows, W, 2.0 / W)
        assert rel_rms(back.cpu(), x) < 1e-5


@pytest.mark.parametrize("W", ROWS)
def test_irfft_rows(ops, W):
    """c2r on the leading (H, W/2+1) slice of wider and taller spectrum planes, plain and with the residual epilogue; Im of bins 0 and
    W/2 is ignored (include/fdn_hip.h), as torch.fft.irfft ignores it."""
    what = _row_route(ops, W, inverse=True)
    rpb = FFT_ROW_ROUTES[W][2]
    H, Hin, Wf = rpb + 1, rpb + 3, W // 2 + 1
    Wfin = Wf + 3
    z = _rnd(2, 1, Hin, Wfin, 2, seed=W)
    assert z[..., 0, 1].abs().min() > 0 and z[..., W // 2, 1].abs().min() > 0
    res = _rnd(2, 1, H, W, seed=W + 1)
    scale = 2.0 / (H * W)
    zc = torch.view_as_complex(z)[:, :, :H, :Wf]
    truth = torch.fft.irfft(zc.to(torch.complex128), n=W, dim=-1) * (W / 2) * scale
    ref32 = torch.fft.irfft(zc, n=W, dim=-1) * (W / 2) * scale
    got = ops.irfft_rows(dev(z), H, W, scale)
    _per_line(got, ref32, truth, (3,), what)
    assert rel_rms(got.cpu(), truth) < 3e-6
    got = ops.irfft_rows(dev(z), H, W, scale, res=dev(res), alpha=0.75)
    _per_line(got, ref32 + 0.75 * res, truth + 0.75 * res.double(), (3,), what + " +res")
    assert rel_rms(got.cpu(), truth + 0.75 * res.double()) < 3e-6


@pytest.mark.parametrize("W", [1280, 320, 1920, 608, 1120])
def test_rfft_rows_misaligned_planned_width(ops, W):
    """A planned width whose input is only 4-byte aligned takes the generic kernel (the planned one loads 8-byte pairs) and is as accurate."""
    assert ops.fft_route(ops.FFT_ROWS, W)["route"] == "planned"
    rows = 7
    buf = _rnd(rows * W + 1, seed=W)
    x = dev(buf)[1:].view(1, 1, rows, W)
    assert x.data_ptr() % 8 == 4
    z = ops.rfft_rows(x)
    xc = buf[1:].view(1, 1, rows, W)
    truth = torch.view_as_real(torch.fft.rfft(xc.double(), dim=-1))
    _per_line(z, torch.view_as_real(torch.fft.rfft(xc, dim=-1)), truth, (3, 4), "rows misaligned planned width")
    assert rel_rms(z.cpu(), truth) < 2e-6


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("H", sorted(H for H, r in FFT_COL_ROUTES.items() if r[0] == "refused"))
def test_cols_refused(ops, H):
    """Columns whose ping-pong buffers and table exceed the LDS of a workgroup: FDN_ERR_UNSUPPORTED from all three modes, no write."""
    _col_route(ops, H)
    lib, s = ops.lib(), ops.stream()
    Wf = 3
    z = dev(torch.full((1, 1, H, Wf, 2), 7.0))
    outs = dev(torch.full((2, 1, 1, H, Wf), -3.0))
    mag, pha = dev(torch.rand(1, 1, H, Wf)), dev(torch.rand(1, 1, H, Wf))
    guide = dev(torch.zeros(1, H, Wf, 8))
    w = dev(torch.ones(1, 3))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.fdn_fft_cols_fwd(p(z), p(outs[0]), p(outs[1]), ctypes.c_long(1), H, Wf, 0, 1, s) == ops.ERR_UNSUPPORTED
    assert lib.fdn_fft_cols_inv_polar(p(mag), p(pha), H, Wf, p(z), ctypes.c_long(1), H, Wf, s) == ops.ERR_UNSUPPORTED
    assert lib.fdn_fft_cols_fcaffn(p(z), p(guide), p(w), p(w), 1, 1, H, Wf, s) == ops.ERR_UNSUPPORTED
    with pytest.raises(RuntimeError, match="code 4"):
        ops.fft_cols_fwd(z, True, True)
    torch.cuda.synchronize()
    assert (z.cpu() == 7.0).all() and (outs.cpu() == -3.0).all()


def test_rows_refused(ops):
    """Rows past the LDS of a workgroup: FDN_ERR_UNSUPPORTED and no write; an odd width: FDN_ERR_ARG (both directions)."""
    lib, s = ops.lib(), ops.stream()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for W in sorted(W for W, r in FFT_ROW_ROUTES.items() if r[0] == "refused"):
        _row_route(ops, W)
        x = dev(_rnd(2, W, seed=W))
        out = dev(torch.full((2, W // 2 + 1, 2), 5.0))
        back = dev(torch.full((2, W), 5.0))
        assert lib.fdn_rfft_rows(p(x), p(out), ctypes.c_long(2), W, ctypes.c_long(0), s) == ops.ERR_UNSUPPORTED
        assert lib.fdn_irfft_rows(p(out), ctypes.c_long(W // 2 + 1), ctypes.c_long(W // 2 + 1), p(back), ctypes.c_long(2), 1, W,
                                  ctypes.c_float(1.0), None, ctypes.c_float(0.0), s) == ops.ERR_UNSUPPORTED
        with pytest.raises(RuntimeError, match="code 4"):
            ops.rfft_rows(x)
        torch.cuda.synchronize()
        assert (out.cpu() == 5.0).all() and (back.cpu() == 5.0).all()
    W = 641
    x = dev(_rnd(2, W + 1, seed=1))
    out = dev(torch.full((2, W // 2 + 2, 2), 5.0))
    assert lib.fdn_rfft_rows(p(x), p(out), ctypes.c_long(2), W, ctypes.c_long(0), s) == 1
    assert lib.fdn_irfft_rows(p(out), ctypes.c_long(W // 2 + 2), ctypes.c_long(W // 2 + 2), p(x), ctypes.c_long(2), 1, W,
                              ctypes.c_float(1.0), None, ctypes.c_float(0.0), s) == 1
    torch.cuda.synchronize()
    assert (out.cpu() == 5.0).all()
