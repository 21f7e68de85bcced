"""CPU: tests/kernel_table.txt names, for every device kernel compiled into libfdn_hip.so, the GPU test files that launch it.

The table is written by `tools/kernel_coverage.py table` from a kernel trace of the GPU suite.  A change that adds a kernel instantiation
fails here until its author has a test that launches it and regenerates the table; one that removes a kernel must drop its row.  A kernel may
be waived only where no test of a few seconds can reach it (a tensor beyond 2 GiB or a 32-bit offset limit, a device count the suite cannot
pose), and at most MAX_WAIVERS rows may say so."""
import importlib.util
import os

import pytest

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "kernel_table.txt")
MAX_WAIVERS = 8


@pytest.fixture(scope="module")
def cov():
    spec = importlib.util.spec_from_file_location("kernel_coverage", os.path.join(ROOT, "tools", "kernel_coverage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def compiled(cov):
    import fdn_hip
    if not os.path.isfile(fdn_hip.lib_path()):
        entry.build()
    return cov.compiled(fdn_hip.lib_path())


def test_kernel_table_is_the_built_library(cov, compiled):
    rows = cov.read_table(TABLE)
    missing, stale = sorted(set(compiled) - set(rows)), sorted(set(rows) - set(compiled))
    assert not missing and not stale, (
        f"{len(missing)} compiled kernels have no row in tests/kernel_table.txt (name the test that launches each, then regenerate the table):\n  "
        + "\n  ".join(f"{k}   {compiled[k][0]}" for k in missing)
        + f"\n{len(stale)} rows name kernels that the library no longer holds:\n  " + "\n  ".join(f"{k}   {rows[k][0]}" for k in stale))
    for k, (dem, _) in compiled.items():
        assert rows[k][0] == dem, (k, rows[k][0], dem)


def test_every_kernel_has_a_host_stub(compiled):
    """a device kernel without a host __device_stub__ is code no launcher refers to: its dispatch line is dead"""
    dead = sorted(dem for dem, stub in compiled.values() if not stub)
    assert not dead, dead


def test_every_row_names_a_gpu_test_file_or_a_waiver(cov):
    rows = cov.read_table(TABLE)
    waived = {k: w for k, (_, w) in rows.items() if w.startswith("WAIVED:")}
    assert len(waived) <= MAX_WAIVERS, sorted(waived)
    for k, w in waived.items():
        assert len(w) > len("WAIVED: ") + 20, f"{k}: a waiver states its reason"
    for k, (dem, where) in rows.items():
        if k in waived:
            continue
        files = where.split()
        assert files, f"{dem}: no test launches it"
        for f in files:
            assert f.startswith("test_gpu_") and os.path.isfile(os.path.join(ROOT, "tests", f)), f"{dem}: {f} is not a GPU test file"


def test_stub_names_map_to_kernel_names(cov):
    f = cov._stub_to_kernel
    assert f("_Z35__device_stub__pack_guidance_kernelPKfS0_") == "_Z20pack_guidance_kernelPKfS0_"
    assert f("_ZN12_GLOBAL__N_135__device_stub__conv3x3_split_kernelILi1ELi4EEEvNS_6C3ArgsEii") == \
        "_ZN12_GLOBAL__N_120conv3x3_split_kernelILi1ELi4EEEvNS_6C3ArgsEii"
    assert cov.template_of("void (anonymous namespace)::conv1x1_kernel<1, 0, 4, true>(fdn_conv1x1_desc, (anonymous namespace)::Geo)") == "conv1x1_kernel"
    assert cov.short("void (anonymous namespace)::k<1, (Pro)2>(int)") == "k<1, (Pro)2>"
