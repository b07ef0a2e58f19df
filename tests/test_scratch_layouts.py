"""The scratch layouts of the tree calls (rrtplanner_amd/csrc/rrt_scratch.h), on the CPU: tests/scratch_layouts/scratch_layouts.cpp
includes that header alone, is compiled with g++ under the address and undefined-behaviour sanitizers and run as a child process.
It prints the bytes and every array of every layout, and writes both ends of every array into a heap block of exactly those bytes.

What is asserted stands here, written out: the byte counts are those the library computed by hand before the layouts were declared
(`rows * 29 + 8` and the like at its reserve calls), the arrays and their order those its comments gave."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "scratch_layouts", "scratch_layouts.cpp")
CSRC = os.path.join(ROOT, "rrtplanner_amd", "csrc")
CAPS = (1, 2, 7, 8, 9, 255, 256, 257, 4097)


def cap8(n):
    return (n + 7) // 8 * 8


# layout -> (bytes of a capacity, the arrays in their order)
EXPECTED = {
    "route_goal": (lambda c: 32 * c + 20, ("length", "raw_off", "fin_off", "cnt", "kept", "err")),
    "route_row": (lambda c: 20 * c, ("row_xy", "row_id", "out_xy", "out_id")),
    "pose_route_goal": (lambda c: 28 * c + 20, ("length", "raw_off", "goal_pt_off", "cnt", "err")),
    "pose_route_row": (lambda c: 29 * c + 8, ("leg_len", "pt_off", "row_xy", "row_id", "npts", "row_h")),
    "pose_cut_goal": (lambda c: 12 * c + 8, ("fin_off", "kept")),
    "pose_cut_row": (lambda c: 9 * c, ("row_xy", "row_id", "row_h")),
    "keep": (lambda c: 16 * c, ("live_vcost", "live_nodes", "live_id")),
    "keep_dubins": (lambda c: 17 * c, ("live_vcost", "live_nodes", "live_id", "live_heading")),
    "keep_tmp": (lambda c: 10 * cap8(c) + 8, ("anc0", "anc1", "ok0", "ok1", "count")),
    "seed_tmp": (lambda c: 4 * (2 * c + 2), ("rank", "new_parent", "err")),
}


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    """{(layout, cap): (bytes, [(array, offset, element size, length)])} as the program printed them; it has run clean under the sanitizers"""
    exe = str(tmp_path_factory.mktemp("scratch_layouts") / "scratch_layouts")
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
            arrays = []
            out[(name, numbers[0])] = (numbers[1], arrays)
        else:
            assert kind == "array", line
            arrays.append((name, *numbers))
    return out


def test_every_layout_at_every_capacity_was_printed(printed):
    assert sorted(printed) == sorted((name, cap) for name in EXPECTED for cap in CAPS)


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_bytes_order_alignment_and_bounds(printed, name):
    nbytes_of, order = EXPECTED[name]
    for cap in CAPS:
        nbytes, arrays = printed[(name, cap)]
        assert nbytes == nbytes_of(cap), (name, cap)
        assert tuple(a[0] for a in arrays) == order, (name, cap)
        end = 0
        for array, offset, size, length in arrays:
            assert length >= 1 and offset % size == 0, (name, cap, array, offset, size)
            assert offset >= end, f"{name} cap={cap}: {array} at {offset} overlaps the array before it, which ends at {end}"
            end = offset + size * length
        assert end <= nbytes, f"{name} cap={cap}: the last array ends at {end} of {nbytes} bytes"
