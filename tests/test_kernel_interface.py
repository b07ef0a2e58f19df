"""CPU: the host units of librrt_hip.so reach the kernels through one interface header and parse no kernel file.

rrtplanner_amd/csrc/rrt_kernel_abi.h holds what the host units (rrt_engine.hip, rrt_tree_calls.hip) and the kernel units
(kernels_tu.hip) share: the structs a kernel takes, the constants the engine sizes by, a declaration of every kernel a host unit
launches.  The kernel files hold definitions only: no macro turns one into a list of declarations.  What is checked:

  (a) no file under csrc names a `*_DECL_ONLY` macro;
  (b) none of the files kernels_tu.hip includes directly, and no `*.inc`, is among the headers the compiler reads for a host unit
      (`hipcc --cuda-host-only -MM` with the Makefile's include flags), and the interface header is among them for both;
  (c) a file that includes only the interface header compiles (`-fsyntax-only`, host and device pass).

The compiler is the Makefile's HIPCC; a missing compiler is a failure, not a skip."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rrtplanner_amd", "csrc")
ABI = "rrt_kernel_abi.h"
HOST_UNITS = ("rrt_engine.hip", "rrt_tree_calls.hip")


def _make_var(name):
    m = re.search(r"^%s\s*[:?]?=\s*(.*)$" % name, open(os.path.join(CSRC, "Makefile")).read(), re.M)
    assert m, f"the Makefile sets no {name}"
    return m.group(1).strip()


def _hipcc():
    return os.environ.get("HIPCC") or _make_var("HIPCC")


def _inc():
    return _make_var("INC").replace("$(ROOT)", ROOT).split()


def _run(args, **kw):
    r = subprocess.run([_hipcc()] + args, cwd=CSRC, capture_output=True, text=True, **kw)
    assert r.returncode == 0, f"{' '.join(args)}\n{r.stderr}"
    return r.stdout


def _definition_files():
    """what kernels_tu.hip includes directly, and every textual part of a kernel body"""
    tu = open(os.path.join(CSRC, "kernels_tu.hip")).read()
    direct = set(re.findall(r'^\s*#\s*include\s+"([^"]+)"', tu, re.M))
    assert direct, "kernels_tu.hip includes no kernel file"
    return direct | {os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.inc"))}


@pytest.fixture(scope="module")
def host_deps():
    """unit -> the base names of the files `hipcc --cuda-host-only -MM` lists for it"""
    out = {}
    for unit in HOST_UNITS:
        text = _run(["--cuda-host-only", "-MM", "-std=c++17"] + _inc() + [unit])
        out[unit] = {os.path.basename(w) for w in text.replace("\\\n", " ").split()[1:]}
    return out


def test_no_decl_only_macro():
    hits = []
    for dirpath, dirnames, files in os.walk(CSRC):
        dirnames[:] = [d for d in dirnames if d != "build"]
        for f in files:
            p = os.path.join(dirpath, f)
            if b"_DECL_ONLY" in open(p, "rb").read():
                hits.append(os.path.relpath(p, CSRC))
    assert hits == []


@pytest.mark.parametrize("unit", HOST_UNITS)
def test_host_unit_parses_no_kernel_file(host_deps, unit):
    deps = host_deps[unit]
    assert unit in deps  # (the list is the compiler's: it names the unit itself)
    assert ABI in deps
    assert ABI not in _definition_files()
    assert sorted(deps & _definition_files()) == []


def test_interface_header_stands_alone(tmp_path):
    src = tmp_path / "abi_only.hip"
    src.write_text(f'#include "{ABI}"\n')
    _run(["--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-Wno-unused-command-line-argument"] + _inc() + [str(src)])
