"""CPU: tests/kernel_table_piqe.txt names, for every device kernel compiled into libfdn_piqe.so, the GPU test files that launch it -
the rule of tests/test_kernel_table_msssim_cpu.py for the library that csrc/piqe.hip is linked into."""
import importlib.util
import os

import pytest

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "kernel_table_piqe.txt")


@pytest.fixture(scope="module")
def cov():
    spec = importlib.util.spec_from_file_location("kernel_coverage", os.path.join(ROOT, "tools", "kernel_coverage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def compiled(cov):
    from fdn_hip import piqe
    if not os.path.isfile(piqe.lib_path()):
        entry.build()
    return cov.compiled(piqe.lib_path())


def test_kernel_table_is_the_built_library(cov, compiled):
    rows = cov.read_table(TABLE)
    assert sorted(rows) == sorted(compiled), (sorted(set(compiled) - set(rows)), sorted(set(rows) - set(compiled)))
    for k, (dem, stub) in compiled.items():
        assert rows[k][0] == dem, (k, rows[k][0], dem)
        assert stub, f"{dem}: no host code launches it"
        assert "piqe_" in dem                                                       # names no other file uses
    assert len(rows) == 2


def test_every_row_names_a_gpu_test_file(cov):
    for k, (dem, where) in cov.read_table(TABLE).items():
        files = where.split()
        assert files, f"{dem}: no test launches it"
        for f in files:
            assert f.startswith("test_gpu_") and os.path.isfile(os.path.join(ROOT, "tests", f)), f"{dem}: {f} is not a GPU test file"


def test_the_other_libraries_hold_none_of_them(cov, compiled):
    """csrc/piqe.hip is linked into no other library of the package: their tables stay what they were"""
    others = sorted(f for f in os.listdir(os.path.join(ROOT, "tests")) if f.startswith("kernel_table") and f.endswith(".txt") and f != os.path.basename(TABLE))
    assert {"kernel_table.txt", "kernel_table_correct.txt", "kernel_table_fusion.txt", "kernel_table_mctf.txt", "kernel_table_motion.txt",
            "kernel_table_msssim.txt", "kernel_table_sharpness.txt"} <= set(others)
    for name in others:
        assert not set(cov.read_table(os.path.join(ROOT, "tests", name))) & set(compiled), name
