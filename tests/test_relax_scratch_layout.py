"""The scratch layout of the relax call (RelaxScratch, rrtplanner_amd/csrc/rrt_scratch.h), on the CPU, as
tests/test_reroot_scratch_layout.py checks RerootScratch: tests/scratch_layouts/relax_layout.cpp includes that header alone, is compiled
with g++ under the address and undefined-behaviour sanitizers and run as a child process.  It prints the bytes and every array of the
layout, and writes both ends of every array into a heap block of exactly those bytes.

The byte count is written out here: one f64 and four 32-bit words per vertex, four 64-bit counters, two words per cell and one more, two
flag arrays of the cell count rounded up to 8, and two of the capacity rounded up to 8."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "scratch_layouts", "relax_layout.cpp")
CSRC = os.path.join(ROOT, "rrtplanner_amd", "csrc")
CAPS = (1, 2, 7, 8, 9, 255, 256, 257, 4097)
CELLS = (1, 9, 4096)
ORDER = ("cost", "stats", "cell_of", "items", "item_xy", "pos_of", "cell_start", "cell_fill", "dirty0", "dirty1", "changed0", "changed1")


def up8(n):
    return (n + 7) // 8 * 8


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    """{(cap, cells): (bytes, [(array, offset, element size, length)])} as the program printed them; it has run clean under the sanitizers"""
    exe = str(tmp_path_factory.mktemp("relax_layout") / "relax_layout")
    # (the sanitizers' runtimes linked into the program itself: it runs the same whatever else the process environment loads)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", "-g", "-I" + CSRC, SRC, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, f"exit {run.returncode}\n{run.stderr[-4000:]}"
    out = {}
    for line in run.stdout.splitlines():
        kind, name, *numbers = line.split()
        numbers = [int(x) for x in numbers]
        if kind == "layout":
            assert name == "relax_tmp"
            arrays = []
            out[(numbers[0], numbers[1])] = (numbers[2], arrays)
        else:
            assert kind == "array", line
            arrays.append((name, *numbers))
    return out


def test_bytes_order_alignment_and_bounds(printed):
    assert sorted(printed) == sorted((cap, cells) for cap in CAPS for cells in CELLS)
    for (cap, cells), (nbytes, arrays) in printed.items():
        assert nbytes == 8 * cap + 8 * 4 + 4 * 4 * cap + 4 * (2 * cells + 1) + 2 * up8(cells) + 2 * up8(cap), (cap, cells)
        assert tuple(a[0] for a in arrays) == ORDER, (cap, cells)
        end = 0
        for array, offset, size, length in arrays:
            assert length >= 1 and offset % size == 0, (cap, cells, array, offset, size)
            assert offset >= end, f"cap={cap} cells={cells}: {array} at {offset} overlaps the array before it, which ends at {end}"
            end = offset + size * length
        assert end <= nbytes, f"cap={cap} cells={cells}: the last array ends at {end} of {nbytes} bytes"
