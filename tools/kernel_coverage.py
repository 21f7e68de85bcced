#!/usr/bin/env python3
"""Which of the library's compiled device kernels does the GPU suite launch?

  kernel_coverage.py symbols <lib.so>                       every compiled kernel: mangled <TAB> demangled
  kernel_coverage.py launched [--lib lib.so] <trace dir>..  the library's kernels that the traces dispatched
  kernel_coverage.py report <lib.so> <trace dir> ...        compiled kernels never launched, by template
  kernel_coverage.py table <lib.so> <trace dir> ... [--waivers old_table]   the rows of tests/kernel_table.txt

`symbols` needs no GPU: it cuts the gfx950 code objects out of the library's .hip_fatbin section (one
clang offload bundle per translation unit) and reads their kernel-descriptor (`.kd`) symbols with the
ROCm `llvm-readelf`.  A kernel without a host `__device_stub__` symbol is marked: no host code can launch it.

The trace directories come from runs of
  rocprofv3 --kernel-trace --mangled-kernels --output-format csv -d <dir>/<test file> -- python -m pytest tests/<test file> ...
one per test file; every `*kernel_trace.csv` below <dir>/<test file> counts for that file (a test that starts
child processes leaves several).  Only names and dispatch names are read, never a kernel's instructions.
"""
import argparse
import csv
import glob
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_LIB = os.path.join(ROOT, "fdn-tip2025_amd", "fdn_hip", "libfdn_hip.so")
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
ARCH = "gfx950"


def _llvm_bin():
    for d in (os.environ.get("ROCM_LLVM_BIN"), os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"),
              "/opt/rocm/lib/llvm/bin"):
        if d and os.path.exists(os.path.join(d, "llvm-readelf")):
            return d
    raise SystemExit("kernel_coverage: no llvm-readelf (set ROCM_PATH or ROCM_LLVM_BIN)")


def _readelf(*args):
    return subprocess.run([os.path.join(_llvm_bin(), "llvm-readelf"), *args], check=True, capture_output=True, text=True).stdout


def _fatbin(lib):
    """Bytes of the .hip_fatbin section."""
    for line in _readelf("-S", "--wide", lib).splitlines():
        m = re.match(r"\s*\[\s*\d+\]\s+\.hip_fatbin\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
        if m:
            off, size = int(m.group(2), 16), int(m.group(3), 16)
            with open(lib, "rb") as f:
                f.seek(off)
                return f.read(size)
    raise SystemExit(f"kernel_coverage: {lib} has no .hip_fatbin section")


def _code_objects(blob):
    """The gfx950 code objects of every uncompressed clang offload bundle in the section."""
    if b"CCOB" in blob[:4] or BUNDLE_MAGIC not in blob:
        raise SystemExit("kernel_coverage: compressed or unknown offload bundle (build without --offload-compress)")
    i = blob.find(BUNDLE_MAGIC)
    while i >= 0:
        (n,) = struct.unpack_from("<Q", blob, i + len(BUNDLE_MAGIC))
        p = i + len(BUNDLE_MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if triple.startswith("hip") and triple.endswith(ARCH) and size:
                yield blob[i + off:i + off + size]
        i = blob.find(BUNDLE_MAGIC, i + 1)


def _kd_names(path, demangle):
    out = []
    for line in _readelf("-s", "--wide", *(["-C"] if demangle else []), path).splitlines():
        f = line.split(None, 7)
        if len(f) < 8 or f[3] != "OBJECT":
            continue
        name = f[7]
        if demangle and name.endswith(" (.kd)"):
            out.append((int(f[1], 16), name[:-6]))
        elif name.endswith(".kd"):
            out.append((int(f[1], 16), name[:-3]))
    return out


def _stub_to_kernel(sym):
    """_Z29__device_stub__foo... -> _Z14foo... (the 15 characters of the prefix leave the length)."""
    s = re.sub(r"(\d+)__device_stub__", lambda m: str(int(m.group(1)) - 15), sym)
    return s.replace("__device_stub__", "")


def compiled(lib):
    """{mangled: (demangled, has_host_stub)} of the library's gfx950 kernels."""
    stubs = set()
    for line in _readelf("-s", "--wide", lib).splitlines():
        if "__device_stub__" in line:
            stubs.add(_stub_to_kernel(line.split()[-1]))
    kernels = {}
    with tempfile.TemporaryDirectory() as tmp:
        for k, co in enumerate(_code_objects(_fatbin(lib))):
            path = os.path.join(tmp, f"co{k}.o")
            with open(path, "wb") as f:
                f.write(co)
            plain = dict(_kd_names(path, False))            # descriptor address -> mangled
            for addr, dem in _kd_names(path, True):
                kernels[plain[addr]] = (dem, plain[addr] in stubs)
    if not kernels:
        raise SystemExit(f"kernel_coverage: no {ARCH} kernel in {lib}")
    return kernels


def launched(dirs, names):
    """{mangled: sorted test files} for the kernels of `names` found in the traces below `dirs`."""
    seen = {}
    for d in dirs:
        files = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
        if not files:
            print(f"kernel_coverage: no *kernel_trace.csv under {d}", file=sys.stderr)
        for path in files:
            rel = os.path.relpath(path, d).split(os.sep)
            test = rel[0] if len(rel) > 1 else os.path.basename(os.path.abspath(d))
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    k = row["Kernel_Name"]
                    k = k[:-3] if k.endswith(".kd") else k
                    if k in names:
                        seen.setdefault(k, set()).add(test)
    return {k: sorted(v) for k, v in seen.items()}


def template_of(demangled):
    """conv1x1_kernel of 'void (anonymous namespace)::conv1x1_kernel<1, 0, 4, true>(fdn_conv1x1_desc, ...)'."""
    s = re.sub(r"^void ", "", demangled).replace("(anonymous namespace)::", "")
    return re.split(r"[<(]", s, 1)[0]


def short(demangled):
    s = re.sub(r"^void ", "", demangled).replace("(anonymous namespace)::", "")
    depth = 0
    for i, c in enumerate(s):               # cut the parameter list, keep the template arguments
        depth += c == "<"
        depth -= c == ">"
        if c == "(" and depth == 0:
            return s[:i]
    return s


def read_table(path):
    rows = {}
    with open(path) as f:
        for line in f:
            if line.strip() and not line.startswith("#"):
                mangled, demangled, where = line.rstrip("\n").split("\t")
                rows[mangled] = (demangled, where)
    return rows


def cmd_symbols(a):
    for k, (dem, stub) in sorted(compiled(a.lib).items()):
        print(f"{k}\t{dem}" + ("" if stub else "\t[no host stub]"))


def cmd_launched(a):
    names = compiled(a.lib)
    for k, tests in sorted(launched(a.traces, names).items()):
        print(f"{k}\t{' '.join(tests)}")


def cmd_report(a):
    names = compiled(a.lib)
    hit = launched(a.traces, names)
    groups = {}
    for k, (dem, stub) in names.items():
        g = groups.setdefault(template_of(dem), [0, []])
        g[0] += 1
        if k not in hit:
            g[1].append(short(dem) + ("" if stub else "   [no host stub: no launcher refers to it]"))
    missing = sum(len(g[1]) for g in groups.values())
    print(f"compiled kernels: {len(names)}   launched: {len(names) - missing}   never launched: {missing}")
    for t, (n, miss) in sorted(groups.items(), key=lambda kv: (-len(kv[1][1]), kv[0])):
        if miss:
            print(f"\n{t}: {len(miss)} of {n}")
            for m in sorted(miss):
                print(f"  {m}")
    return 0


def cmd_table(a):
    names = compiled(a.lib)
    hit = launched(a.traces, names)
    waived = {k: w for k, (_, w) in read_table(a.waivers).items() if w.startswith("WAIVED:")} if a.waivers else {}
    print("# one row per kernel compiled into libfdn_hip.so: mangled <TAB> demangled <TAB> test files that launch it, or WAIVED: reason")
    print("# generated by tools/kernel_coverage.py table from a traced run of the GPU suite; tests/test_kernel_table_cpu.py holds it to the build")
    bad = 0
    for k, (dem, _) in sorted(names.items()):
        where = " ".join(hit[k]) if k in hit else waived.get(k, "")
        if not where:
            where, bad = "UNLAUNCHED", bad + 1
        print(f"{k}\t{dem}\t{where}")
    if bad:
        print(f"kernel_coverage: {bad} kernels neither launched nor waived", file=sys.stderr)
    return 1 if bad else 0


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = p.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("symbols")
    s.add_argument("lib")
    s.set_defaults(fn=cmd_symbols)
    s = sub.add_parser("launched")
    s.add_argument("--lib", default=DEFAULT_LIB)
    s.add_argument("traces", nargs="+")
    s.set_defaults(fn=cmd_launched)
    s = sub.add_parser("report")
    s.add_argument("lib")
    s.add_argument("traces", nargs="+")
    s.set_defaults(fn=cmd_report)
    s = sub.add_parser("table")
    s.add_argument("lib")
    s.add_argument("traces", nargs="+")
    s.add_argument("--waivers", help="an earlier table whose WAIVED rows are kept")
    s.set_defaults(fn=cmd_table)
    a = p.parse_args()
    sys.exit(a.fn(a) or 0)


if __name__ == "__main__":
    main()
