"""The scratch layout of the reroot_poses call beyond those of relax_poses (PoseRerootScratch, rrtplanner_amd/csrc/rrt_scratch.h), on the
CPU, as tests/test_pose_relax_scratch_layout.py checks PoseRelaxScratch: tests/scratch_layouts/pose_reroot_layout.cpp includes that header
alone, is compiled with g++ under the address and undefined-behaviour sanitizers and run as a child process.  It prints the bytes and
every array of the layout, and writes both ends of every array into a heap block of exactly those bytes.

The byte count is written out here: three 4-byte arrays per vertex, and one byte array of the capacity rounded up to 8."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "scratch_layouts", "pose_reroot_layout.cpp")
CSRC = os.path.join(ROOT, "rrtplanner_amd", "csrc")
CAPS = (1, 2, 7, 8, 9, 255, 256, 257, 4097)
ORDER = ("f_nodes", "f_parent", "f_id", "f_heading")


def up8(n):
    return (n + 7) // 8 * 8


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    """{cap: (bytes, [(array, offset, element size, length)])} as the program printed them; it has run clean under the sanitizers"""
    exe = str(tmp_path_factory.mktemp("pose_reroot_layout") / "pose_reroot_layout")
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
            assert name == "pose_reroot_tmp"
            arrays = []
            out[numbers[0]] = (numbers[1], arrays)
        else:
            assert kind == "array", line
            arrays.append((name, *numbers))
    return out


def test_bytes_order_alignment_and_bounds(printed):
    assert sorted(printed) == sorted(CAPS)
    for cap, (nbytes, arrays) in printed.items():
        assert nbytes == 3 * 4 * cap + up8(cap), cap
        assert tuple(a[0] for a in arrays) == ORDER, cap
        end = 0
        for array, offset, size, length in arrays:
            assert length >= 1 and offset % size == 0, (cap, array, offset, size)
            assert offset >= end, f"cap={cap}: {array} at {offset} overlaps the array before it, which ends at {end}"
            end = offset + size * length
        assert end <= nbytes, f"cap={cap}: the last array ends at {end} of {nbytes} bytes"
