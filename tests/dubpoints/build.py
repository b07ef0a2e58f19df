"""Builds tests/dubpoints/libdubpoints.so (see dubpoints.c: test infrastructure, the points of one Dubins leg on the host).  gcc with
the flags of oracle/Makefile, -ffp-contract=off among them; well under a second."""
import ctypes as C
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(HERE, "libdubpoints.so")
SRC = os.path.join(HERE, "dubpoints.c")
INCLUDE = os.path.join(ROOT, "include")


def oracle_cflags():
    """the CFLAGS of oracle/Makefile, so that the helper and the oracle are compiled alike"""
    m = re.search(r"^CFLAGS\s*\?=\s*(.*)$", open(os.path.join(ROOT, "oracle", "Makefile")).read(), re.M)
    assert m and "-ffp-contract=off" in m.group(1), "oracle/Makefile sets no CFLAGS with -ffp-contract=off"
    return m.group(1).split()


def build(force=False):
    deps = [SRC, os.path.join(INCLUDE, "rrt_dubins_points.h"), os.path.join(INCLUDE, "rrt_dubins.h")]
    if force or not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["gcc"] + oracle_cflags() + ["-shared", "-I" + INCLUDE, SRC, "-o", LIB, "-lm"])
    return LIB


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.dubpoints_leg.argtypes = [C.c_double] * 7 + [C.c_void_p, C.c_int32, C.c_void_p]
        _lib.dubpoints_leg.restype = C.c_int32
    return _lib


if __name__ == "__main__":
    print(build(force=True))
