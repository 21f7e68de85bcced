"""CPU: the host side of the Fourier evaluation - the entry points of include/fdn_spectral.h (version, prototype table, argument checks
before any launch, the band counts, which are host arithmetic), the restatement of tests/spectral_ref.py judged on its own (Parseval and
amp + pha = total), what fdn_hip.spectral refuses, and the argument parsing of calculate_fourier_metrics.py and validate_fdn.py --fourier.
No GPU compute."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as entry  # noqa: F401  (puts the package on sys.path)
import spectral_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fdn_spectral_abi_version", "fdn_fft_cols_c2c", "fdn_spectrum_band_counts", "fdn_spectrum_pair_bands_ws", "fdn_spectrum_pair_bands"]
SHAPES = [(2, 2), (7, 10), (45, 64), (34, 38), (736, 1280), (4096, 10240)]
BANDS = [1, 8, 32]


@pytest.fixture(scope="module")
def lib():
    import fdn_hip
    if not os.path.isfile(fdn_hip.lib_path()):
        entry.build()
    return fdn_hip.lib()


def test_version_and_prototype_table(lib):
    """the entry points of include/fdn_spectral.h in the one table (tests/test_host_cpu.py holds it to the headers): names, signatures"""
    from fdn_hip._abi import HEADERS, PROTOTYPES
    assert HEADERS["fdn_spectral.h"] == NAMES
    assert PROTOTYPES["fdn_fft_cols_c2c"] == ("I", ["P", "L", "I", "I", "P"])
    assert PROTOTYPES["fdn_spectrum_band_counts"] == ("I", ["I", "I", "I", "P"])
    assert PROTOTYPES["fdn_spectrum_pair_bands_ws"] == ("L", ["L", "I", "I", "I"])
    assert PROTOTYPES["fdn_spectrum_pair_bands"] == ("I", ["P", "P", "P", "P", "L", "I", "I", "L", "I", "P"])
    assert lib.fdn_spectrum_pair_bands_ws.restype == ctypes.c_long
    assert lib.fdn_spectrum_pair_bands.argtypes == [ctypes.c_void_p] * 4 + [ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.c_int,
                                                    ctypes.c_void_p]


BAD = [dict(planes=0), dict(planes=-1), dict(H=0), dict(H=-3), dict(H=4097), dict(W=37), dict(W=0), dict(W=1), dict(W=-2), dict(W=10242),
       dict(W=10241), dict(nb=0), dict(nb=-1), dict(nb=33), dict(row_bins=19), dict(row_bins=1), dict(row_bins=-1)]


def test_entry_points_validate_arguments_without_gpu(lib):
    """every refusal of include/fdn_spectral.h is FDN_ERR_ARG = 1 before any launch (this machine has no GPU to launch on); the workspace
    query answers 0 to the same sizes"""
    p = ctypes.c_void_p(64)                          # never dereferenced: every call below fails its argument check
    counts = (ctypes.c_long * 33)()

    def pair(za=p, zb=p, out=p, ws=p, planes=1, H=34, W=38, row_bins=0, nb=8):
        return lib.fdn_spectrum_pair_bands(za, zb, out, ws, planes, H, W, row_bins, nb, None)

    for key in ("za", "zb", "out", "ws"):
        assert pair(**{key: None}) == 1, key
    for kw in BAD:
        assert pair(**kw) == 1, kw
        args = dict(planes=1, H=34, W=38, nb=8)
        args.update({k: v for k, v in kw.items() if k != "row_bins"})
        if "row_bins" not in kw:
            assert lib.fdn_spectrum_pair_bands_ws(args["planes"], args["H"], args["W"], args["nb"]) == 0, kw
            if "planes" not in kw:
                assert lib.fdn_spectrum_band_counts(args["H"], args["W"], args["nb"], counts) == 1, kw
    assert lib.fdn_spectrum_band_counts(34, 38, 8, None) == 1
    n = lib.fdn_spectrum_pair_bands_ws(1, 34, 38, 8)
    assert n > 0 and n % 45 == 0 and lib.fdn_spectrum_pair_bands_ws(6, 34, 38, 8) == 6 * n
    assert lib.fdn_spectrum_pair_bands_ws(24, 4096, 10240, 32) > 0 and lib.fdn_spectrum_pair_bands_ws(1, 1, 2, 1) > 0
    # the column pass
    assert lib.fdn_fft_cols_c2c(None, 1, 34, 20, None) == 1
    for planes, H, Wf in ((0, 34, 20), (-1, 34, 20), (1, 0, 20), (1, -1, 20), (1, 34, 0), (1, 34, -1)):
        assert lib.fdn_fft_cols_c2c(p, planes, H, Wf, None) == 1, (planes, H, Wf)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_band_counts(lib, shape):
    """fdn_spectrum_band_counts against the yardstick: the integer rule written independently on arrays and, at the small shapes, exact
    rational arithmetic bin by bin; the counts sum to H W"""
    from fdn_hip import spectral
    H, W = shape
    for nb in BANDS:
        got = spectral.band_counts(H, W, nb)
        assert len(got) == nb + 1 and sum(got) == H * W and got[0] == 1, (nb, got)
        assert got == ref.band_counts(H, W, nb), nb
        if H * W <= 45 * 64:
            assert got == ref.band_counts_slow(H, W, nb), nb
    if shape == (2, 2):
        assert spectral.band_counts(2, 2, 8) == [1, 0, 0, 0, 0, 0, 0, 0, 3]             # rho >= 0.5 everywhere: empty bands between


def test_band_edges_go_to_the_upper_band():
    """H = W = 8, nb = 4: bin (1, 0) has 2 nb rho = 1 exactly and lies in band 2, so band 1 (2 nb rho < 1) is empty; were the edge to fall
    to the lower band, band 1 would hold (1,0), (7,0) and the pair (0,1), 4 bins by weight.  Likewise on every ring of a square image."""
    from fdn_hip import spectral
    assert ref.band_of(1, 0, 8, 8, 4) == 2 and ref.band_of(0, 1, 8, 8, 4) == 2 and ref.band_of(0, 0, 8, 8, 4) == 0
    assert ref.band_of(4, 4, 8, 8, 4) == 4 and ref.band_of(7, 0, 8, 8, 4) == 2 and ref.band_of(2, 0, 8, 8, 4) == 3
    got = spectral.band_counts(8, 8, 4)
    assert got == ref.band_counts_slow(8, 8, 4) and got[1] == 0 and got[2] == 4 + 4, got     # (1,0) (7,0) (0,1)x2 and the four (1,1)-type bins
    # axis bins k of an N x N image with nb bands sit exactly on an edge whenever 2 nb k / N is an integer
    for N, nb in ((16, 8), (64, 32), (64, 8), (40, 5), (4096, 32)):
        edges = [k for k in range(1, N // 2 + 1) if (2 * nb * k) % N == 0]
        assert edges
        for k in edges:
            assert ref.band_of(k, 0, N, N, nb) == ref.band_of(0, k, N, N, nb) == 1 + min(2 * nb * k // N, nb - 1)
        if N <= 64:
            assert spectral.band_counts(N, N, nb) == ref.band_counts_slow(N, N, nb) == ref.band_counts(N, N, nb)
    # an edge off the axes: the Pythagorean bin (3, 4) of a 20 x 20 image has rho = 0.25, so 2 nb rho = 4 exactly at nb = 8 -> band 5
    assert ref.band_of(3, 4, 20, 20, 8) == 5 and ref.band_map(20, 20, 8)[3, 4] == 5
    assert spectral.band_counts(20, 20, 8) == ref.band_counts_slow(20, 20, 8)


def test_restatement_on_its_own():
    """Parseval (the total over the bands / (H W)^2 is the squared error of the pair, the energy likewise) and amp + pha = total per band,
    to 1e-12 relative; a gain error is nearly all amplitude, a displacement all phase"""
    for (h, w), seed in (((7, 10), 1), ((45, 64), 2), ((34, 38), 3)):
        b = ref.textured(h, w, seed).transpose(2, 0, 1) / 255.0
        g = np.random.default_rng(seed)
        a = np.clip(0.8 * b + g.normal(0, 0.05, b.shape), 0, 1)
        for nb in BANDS:
            s = ref.pair_bands(a, b, nb)
            assert s.shape == (3, nb + 1, 5)
            sse = ((a - b) ** 2).sum(axis=(1, 2))
            assert np.allclose(s[:, :, 0].sum(axis=1) / (h * w) ** 2, sse / (h * w), rtol=1e-12, atol=0)
            assert np.allclose(s[:, :, 3].sum(axis=1) / (h * w) ** 2, (b ** 2).sum(axis=(1, 2)) / (h * w), rtol=1e-12, atol=0)
            assert np.allclose(s[:, :, 1] + s[:, :, 2], s[:, :, 0], rtol=1e-12, atol=0)
            m = ref.metrics(s, h, w)
            assert abs(m["mse"] - ((a - b) ** 2).mean()) <= 1e-12 * m["mse"]
            assert abs(m["amp_share"] + m["pha_share"] - 1.0) <= 1e-15 and abs(sum(bd["share"] for bd in m["bands"]) - 1.0) <= 1e-12
            assert abs(m["fft_l1"] - ref.fft_l1(a, b)) <= 1e-12 * m["fft_l1"]
            assert abs(m["dc_share"] - h * w * ((a - b).mean(axis=(1, 2)) ** 2).sum() / ((a - b) ** 2).sum()) <= 1e-12      # the mean offset's part
        m = ref.metrics(ref.pair_bands(0.5 * b, b, 8), h, w)
        assert m["pha_share"] <= 1e-12 and m["psnr_pha"] > m["psnr"] + 120
        m = ref.metrics(ref.pair_bands(np.roll(b, (3, 5), axis=(1, 2)), b, 8), h, w)
        assert m["amp_share"] <= 1e-12
        m = ref.metrics(ref.pair_bands(b, b, 8), h, w)
        assert m["mse"] == 0 and m["psnr"] == float("inf") and m["fft_l1"] == 0 and m["psnr_amp"] == float("inf")
        # |X|^2 - sqrt(|X|^2)^2 is a rounding error of at most a few 2^-53 |X|^2 per bin, not 0: the phase "error" of two equal images is
        # below 4 * 2^-52 of the image's energy (mean b^2 <= 1: 150 dB), and the kernel holds every bin's term at or below the bin's total
        assert m["psnr_pha"] > 150


def test_derived_figures_are_the_restatements():
    """fdn_hip.spectral.metrics_from_sums against tests/spectral_ref.py metrics on the same sums (two summation orders: 1e-12)"""
    from fdn_hip import spectral
    b = ref.textured(34, 38, 5).transpose(2, 0, 1) / 255.0
    a = np.clip(0.7 * b + 0.02, 0, 1)
    s = ref.pair_bands(a, b, 8)
    got, want = spectral.metrics_from_sums(s, 34, 38), ref.metrics(s, 34, 38)
    assert set(got) == set(want) and len(got["bands"]) == 9
    for k in want:
        if k != "bands":
            assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), k
    for g, w in zip(got["bands"], want["bands"]):
        for k in w:
            assert abs(g[k] - w[k]) <= 1e-12 * abs(w[k]), k
    assert len(spectral.csv_header(8)) == len(spectral.csv_row(got)) == 8 + 4 * 9
    assert [float(v) for v in spectral.csv_row(got)][:8] == [got[k] for k in ("mse", "psnr", "amp_share", "pha_share", "dc_share", "psnr_amp", "psnr_pha", "fft_l1")]
    same = spectral.metrics_from_sums(np.zeros((3, 9, 5)), 34, 38)
    assert same["psnr"] == same["psnr_amp"] == float("inf") and math.isnan(same["amp_share"]) and math.isnan(same["bands"][3]["rel_err"])


def test_wrappers_refuse():
    """no host fallback: a CPU tensor, a wrong dtype, mismatched shapes, an odd width, bad band counts - FdnHipError naming the problem"""
    from fdn_hip import FdnHipError, spectral
    x = torch.zeros(1, 3, 34, 38)
    for f in (lambda: spectral.pair_bands(x, x), lambda: spectral.fourier_metrics(x, x), lambda: spectral.rfft2(x)):
        with pytest.raises(FdnHipError, match="ROCm"):
            f()
    with pytest.raises(FdnHipError, match="torch tensor"):
        spectral.rfft2(np.zeros((4, 4), np.float32))
    with pytest.raises(FdnHipError, match="ROCm"):
        spectral.spectrum_pair_bands(torch.zeros(1, 34, 20, dtype=torch.complex64), torch.zeros(1, 34, 20, dtype=torch.complex64), 34, 38)
    for bands in (0, 33, -1, 2.5, None, True):
        with pytest.raises(FdnHipError, match="bands"):
            spectral.pair_bands(x, x, bands=bands)
        with pytest.raises(FdnHipError, match="bands"):
            spectral.band_counts(34, 38, bands)
        with pytest.raises(FdnHipError, match="bands"):
            spectral.calculate_fourier(np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4, 3), np.uint8), bands=bands)
    for H, W, word in ((34, 37, "odd width"), (0, 38, "height"), (4097, 38, "height"), (34, 10242, "width"), (34, 0, "width")):
        with pytest.raises(FdnHipError, match=word):
            spectral.band_counts(H, W, 8)
    u = np.zeros((6, 8, 3), np.uint8)
    with pytest.raises(FdnHipError, match="shapes are different"):
        spectral.calculate_fourier(u, np.zeros((6, 10, 3), np.uint8))
    with pytest.raises(FdnHipError, match="uint8"):
        spectral.calculate_fourier(u.astype(np.float32), u.astype(np.float32))
    if not torch.cuda.is_available():
        with pytest.raises(FdnHipError, match="ROCm"):
            spectral.calculate_fourier(u, u)
        return
    dev = torch.device("cuda:0")                      # with a device the remaining checks are reachable too; all raise before any launch
    y = x.to(dev)
    with pytest.raises(FdnHipError, match="float32"):
        spectral.pair_bands(y.double(), y.double())
    with pytest.raises(FdnHipError, match="shapes are different"):
        spectral.pair_bands(y, y[:, :, :, :36].contiguous())
    with pytest.raises(FdnHipError, match="odd width"):
        spectral.pair_bands(y[..., :37], y[..., :37])
    with pytest.raises(FdnHipError, match="odd width"):
        spectral.rfft2(y[..., :37])
    with pytest.raises(FdnHipError, match="B, C, H, W"):
        spectral.pair_bands(y[0], y[0])
    with pytest.raises(FdnHipError, match="odd width"):
        spectral.calculate_fourier(np.zeros((6, 9, 3), np.uint8), np.zeros((6, 9, 3), np.uint8))


def test_command_line_parsing(tmp_path):
    """calculate_fourier_metrics.py: defaults, the bounds of --bands and --batch, unequal globs; validate_fdn.py: without --fourier every
    attribute it had is what it was, with it the two new ones are set"""
    from PIL import Image
    import calculate_fourier_metrics as tool
    import validate_fdn
    for d in ("lq", "gt", "rs"):
        (tmp_path / d).mkdir()
        for i in range(2):
            Image.fromarray(np.zeros((40, 72, 3), np.uint8)).save(tmp_path / d / f"f{i}.png")
    gt, rs, lq = (str(tmp_path / d / "*.png") for d in ("gt", "rs", "lq"))
    a = tool.parse_args(["--gt", gt, "--restored", rs])
    assert (a.bands, a.csv, a.batch, a.device) == (8, None, 8, "cuda:0")
    assert a.pairs == [(str(tmp_path / "gt" / f"f{i}.png"), str(tmp_path / "rs" / f"f{i}.png")) for i in range(2)]
    a = tool.parse_args(["--gt", gt, "--restored", rs, "--bands", "32", "--csv", "x.csv", "--batch", "3", "--device", "cuda:1"])
    assert (a.bands, a.csv, a.batch, a.device) == (32, "x.csv", 3, "cuda:1")
    for extra in (["--bands", "0"], ["--bands", "33"], ["--batch", "0"], ["--bands", "x"]):
        with pytest.raises(SystemExit):
            tool.parse_args(["--gt", gt, "--restored", rs] + extra)
    for argv in (["--gt", gt], ["--restored", rs], ["--gt", gt, "--restored", str(tmp_path / "rs" / "f0.png")],
                 ["--gt", str(tmp_path / "none*"), "--restored", rs]):
        with pytest.raises(SystemExit):
            tool.parse_args(argv)
    line = tool.fourier_line({"amp_share": 0.25, "pha_share": 0.75, "dc_share": 0.125, "fft_l1": 2.0})
    assert line == "Amp: 0.250000, Pha: 0.750000, DC: 0.125000, FFT-L1: 2.000000"
    assert tool.mean_of([1.0, float("nan"), 3.0]) == 2.0 and math.isnan(tool.mean_of([float("nan")]))

    base = ["--fdn", "x.pth", "--lq", lq, "--gt", gt]
    a = validate_fdn.parse_args(base)
    was = dict(fdn="x.pth", lpnet=None, lq=lq, gt=gt, variant="lolblur", ratio="gt", crop_border=0, output=None, csv=None, batch=8,
               device="cuda:0", tile=None, tile_overlap=0, tile_ratio="tile", tile_blend=a.tile_blend, ensemble=a.ensemble, dest=None,
               pairs=[(str(tmp_path / "lq" / f"f{i}.png"), str(tmp_path / "gt" / f"f{i}.png")) for i in range(2)])
    now = vars(a)
    assert {k: now[k] for k in was} == was and set(now) - set(was) == {"fourier", "fourier_bands"}
    assert a.fourier is False and a.fourier_bands == 8
    a = validate_fdn.parse_args(base + ["--fourier", "--fourier-bands", "4"])
    assert a.fourier is True and a.fourier_bands == 4
    for bad in ("0", "33"):
        with pytest.raises(SystemExit):
            validate_fdn.parse_args(base + ["--fourier", "--fourier-bands", bad])
