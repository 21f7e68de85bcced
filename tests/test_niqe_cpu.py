"""NIQE on the host: the numpy restatement (tests/niqe_ref.py) against the reference's own numbers (tests/golden/niqe.npz), the search
tables fdn_hip.metrics builds for the kernel, the parameter lookup, the host-side MVG fit and the CLI's decoding rules.  No GPU."""
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import niqe_ref as R
from fdn_hip import FdnHipError, metrics

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture(HERE)


@pytest.fixture(scope="module")
def tab():
    return R.tables()


@pytest.mark.parametrize("name", ["tex", "crop", "dark", "hw", "gray", "big", "planes"])
def test_restatement_matches_reference(fx, tab, name):
    z, cases, params, image = fx
    c = cases[name]
    q, d = R.niqe(image(name), params, c["crop_border"], c["input_order"], c["convert_to"], tab)
    assert abs(q / c["niqe"] - 1) < 1e-5, (q, c["niqe"])
    same = []
    for s in (1, 2):
        want, got = z[f"{name}_feat{s}"], d[f"feat{s}"]
        assert want.shape == got.shape
        assert np.array_equal(np.isnan(want), np.isnan(got))
        sm, dmax, worst = R.compare_feats(got, want, tab)
        assert dmax <= 1 and worst <= 1e-6, (s, dmax, worst)
        same.append(sm)
    assert np.concatenate(same).mean() >= 0.99
    if name == "planes":
        assert np.array_equal(d["plane"], z["planes_y"])
        for s in (1, 2):
            assert np.abs(d[f"mscn{s}"] - z[f"planes_mscn{s}"]).max() <= 1e-6


def test_nan_quirk_in_fixture(fx):
    """the under-exposed case has blocks with no negative (or positive) coefficient: alpha = 0.2 (np.argmin over NaN) and NaN betas"""
    z, cases, _, _ = fx
    f = np.concatenate([z["dark_feat1"], z["dark_feat2"]], axis=1)
    dropped = np.nonzero(np.isnan(f).any(axis=1))[0]
    assert dropped.tolist() == cases["dark"]["dropped_rows"] and len(dropped) > 0
    assert np.isclose(f[dropped][:, [0, 18]], 0.2, rtol=0, atol=1e-12).any()
    assert np.isnan(f[dropped][:, 1]).any()


@pytest.mark.parametrize("name", ["tex", "dark", "big"])
def test_host_fit_reproduces_reference(fx, name):
    """metrics.niqe_score on the reference's own features gives the reference's score: same calls, float64"""
    z, cases, params, _ = fx
    dist = np.concatenate([z[f"{name}_feat1"], z[f"{name}_feat2"]], axis=1)
    q = metrics.niqe_score(dist, params["mu_pris_param"], params["cov_pris_param"])
    assert abs(q / cases[name]["niqe"] - 1) < 1e-12


def test_host_fit_refuses_too_few_rows(fx):
    z, _, params, _ = fx
    dist = np.concatenate([z["dark_feat1"], z["dark_feat2"]], axis=1)
    bad = dist.copy()
    bad[1:, 1] = np.nan
    with pytest.raises(FdnHipError, match="complete"):
        metrics.niqe_score(bad, params["mu_pris_param"], params["cov_pris_param"])


def test_table_grid_is_the_references_arange():
    t = metrics.niqe_tables()
    assert t.shape == (4, 9801) and t.dtype == np.float64
    assert np.array_equal(t[0], np.arange(0.2, 10.001, 0.001))
    assert not np.array_equal(t[0], 0.2 + np.arange(9801) * 0.001)     # the grid is not this one, and the kernel reads gam from here
    assert (np.diff(t[1]) > 0).all()                                     # r_gam increases: the kernel's nearest-entry search holds


def test_tables_against_scipy_gamma():
    sp = pytest.importorskip("scipy.special")
    t = metrics.niqe_tables()
    gam = np.arange(0.2, 10.001, 0.001)
    rec = np.reciprocal(gam)
    r_gam = np.square(sp.gamma(rec * 2)) / (sp.gamma(rec) * sp.gamma(rec * 3))
    assert np.abs(t[1] / r_gam - 1).max() < 1e-13
    assert np.abs(t[2] / np.sqrt(sp.gamma(1 / gam) / sp.gamma(3 / gam)) - 1).max() < 1e-13
    assert np.abs(t[3] / (sp.gamma(2 / gam) / sp.gamma(1 / gam)) - 1).max() < 1e-13


def test_params_found_through_basicsr_path(fx, tmp_path, monkeypatch):
    import basicsr
    _, _, params, _ = fx
    own = [d for d in basicsr.__path__ if os.path.abspath(d).startswith(os.path.dirname(HERE))]
    monkeypatch.setattr(basicsr, "__path__", list(own))
    with pytest.raises(FdnHipError, match="params="):
        metrics.niqe_params(None)
    stub = tmp_path / "checkout" / "basicsr" / "metrics"
    stub.mkdir(parents=True)
    np.savez(stub / "niqe_pris_params.npz", **params)
    monkeypatch.setattr(basicsr, "__path__", list(own) + [str(stub.parent)])
    mu, cov, win = metrics.niqe_params(None)
    assert np.array_equal(mu, params["mu_pris_param"]) and np.array_equal(cov, params["cov_pris_param"])
    assert np.array_equal(win, params["gaussian_window"])


def test_params_mapping_and_path(fx, tmp_path):
    _, _, params, _ = fx
    p = tmp_path / "p.npz"
    np.savez(p, **params)
    a, b = metrics.niqe_params(str(p)), metrics.niqe_params(params)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    with pytest.raises(FdnHipError):
        metrics.niqe_params({"mu_pris_param": params["mu_pris_param"]})


def test_refuses_cpu_and_wrong_dtype(fx):
    _, _, params, _ = fx
    with pytest.raises(FdnHipError):
        metrics.calculate_niqe(torch.zeros(3, 96, 96), params=params)
    with pytest.raises(FdnHipError):
        metrics.calculate_niqe(np.zeros((3, 96, 96), np.float32), params=params)


def _png16(path, h=4, w=5):
    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xffffffff)
    raw = b"".join(b"\0" + np.full((w, 3), 1000, ">u2").tobytes() for _ in range(h))
    path.write_bytes(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw))
                     + chunk(b"IEND", b""))


def test_cli_decoding(tmp_path):
    from PIL import Image
    import calculate_niqe as cli
    rgb = np.random.default_rng(0).integers(0, 256, (6, 7, 3), dtype=np.uint8)
    Image.fromarray(rgb).save(tmp_path / "a.png")
    x = cli.load_bgr(tmp_path / "a.png")
    assert x.dtype == np.float32 and np.array_equal(x, rgb[..., ::-1].transpose(2, 0, 1))        # B, G, R
    Image.fromarray(rgb[..., 0]).save(tmp_path / "g.png")
    assert np.array_equal(cli.load_bgr(tmp_path / "g.png"), rgb[None, ..., 0])
    rgba = np.concatenate([rgb, np.full((6, 7, 1), 9, np.uint8)], axis=2)
    Image.fromarray(rgba).save(tmp_path / "c.png")
    with pytest.raises(ValueError, match="alpha"):
        cli.load_bgr(tmp_path / "c.png")
    assert np.array_equal(cli.load_bgr(tmp_path / "c.png", drop_alpha=True), x)
    Image.fromarray(np.zeros((4, 5), np.uint16)).save(tmp_path / "d.png")
    with pytest.raises(ValueError, match="16-bit"):
        cli.load_bgr(tmp_path / "d.png")
    _png16(tmp_path / "e.png")
    with pytest.raises(ValueError, match="16-bit"):
        cli.load_bgr(tmp_path / "e.png")
    assert [os.path.basename(p) for p in cli.list_images(str(tmp_path))] == ["a.png", "c.png", "d.png", "e.png", "g.png"]
