"""CPU: resource use of the split team kernels, read from the gfx950 code objects inside the built librrt_hip.so.

The committer of a pipelined team runs as a workgroup of its own (rrt_block_commit_kernel, 8 waves), so that it is compiled for
256 vector registers instead of the 128 of a 16-wave workgroup.  Its speed follows its register allocation: it must use no
private (scratch) memory at all -- neither spilled vector registers nor scalar registers spilled to memory -- and at most
256 VGPRs.  The kernel descriptors (`<kernel>.kd`, AMDGPU code-object v5) carry both figures."""
import os
import struct

import pytest

from rrtplanner_amd import _ffi

BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
TEAMS = ((64, 1), (32, 2), (16, 4), (8, 8))


def _mangled(kind, g, bsm):
    name = {"commit": "rrt_block_commit_kernel", "work": "rrt_block_work_kernel"}[kind]
    return f"_ZN6rrtdev{len(name)}{name}ILi{g}ELi{bsm}ELb0EEEvNS_9BatchViewE"


def _sections(elf):
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)
    heads = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + k * shentsize) for k in range(shnum)]
    names = heads[shstrndx]
    out = {}
    for h in heads:
        nm = elf[names[4] + h[0]:elf.index(b"\0", names[4] + h[0])].decode()
        out[nm] = h
    return out, heads


def _gfx950_code_objects(so):
    """The device ELF images of every offload bundle of the library (one per translation unit)."""
    secs, _ = _sections(so)
    fat = secs[".hip_fatbin"]
    blob = so[fat[4]:fat[4] + fat[5]]
    images = []
    pos = blob.find(BUNDLE_MAGIC)
    while pos >= 0:
        n, = struct.unpack_from("<Q", blob, pos + 24)
        p = pos + 32
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "gfx950" in triple:
                images.append(blob[pos + off:pos + off + size])
        pos = blob.find(BUNDLE_MAGIC, pos + 1)
    return images


def _kernel_descriptors(so):
    """{symbol: 64-byte kernel descriptor} of every kernel in the library's gfx950 code objects."""
    kds = {}
    for elf in _gfx950_code_objects(so):
        secs, heads = _sections(elf)
        symtab, strtab = secs[".symtab"], secs[".strtab"]
        for k in range(symtab[5] // 24):
            st_name, st_info, st_other, st_shndx, st_value, st_size = struct.unpack_from("<IBBHQQ", elf, symtab[4] + 24 * k)
            nm = elf[strtab[4] + st_name:elf.index(b"\0", strtab[4] + st_name)].decode()
            if nm.endswith(".kd") and st_shndx < len(heads):
                sh = heads[st_shndx]
                at = sh[4] + (st_value - sh[3])
                kds[nm[:-3]] = elf[at:at + 64]
    return kds


@pytest.fixture(scope="module")
def kds():
    if not os.path.exists(_ffi.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    with open(_ffi.LIB_PATH, "rb") as f:
        return _kernel_descriptors(f.read())


def _private_bytes(kd):
    return struct.unpack_from("<I", kd, 4)[0]  # private_segment_fixed_size: scratch bytes per work-item


def _vgprs(kd):
    rsrc1, = struct.unpack_from("<I", kd, 48)  # compute_pgm_rsrc1: granulated VGPR count in bits 0-5, granules of 8 on gfx950
    return ((rsrc1 & 0x3F) + 1) * 8


def test_descriptors_are_read():
    """The reader finds the kernels it should (a sanity check of the parser on the one-body kernel of config 2's team)."""
    with open(_ffi.LIB_PATH, "rb") as f:
        kds = _kernel_descriptors(f.read())
    one = "_ZN6rrtdev23rrt_expand_block_kernelILi64ELi1ELb1ELb0EEEvNS_9BatchViewE"
    assert one in kds and _vgprs(kds[one]) <= 128  # a 16-wave workgroup: the 128-register cap


@pytest.mark.parametrize("g,bsm", TEAMS, ids=[f"{g}+1" for g, _ in TEAMS])
def test_committer_kernel_has_no_scratch_and_at_most_256_vgprs(kds, g, bsm):
    name = _mangled("commit", g, bsm)
    assert name in kds, f"{name} is not in {_ffi.LIB_PATH}"
    assert _private_bytes(kds[name]) == 0, "the committer spills to scratch memory"
    assert 128 < _vgprs(kds[name]) <= 256


@pytest.mark.parametrize("g,bsm", TEAMS, ids=[f"{g}+1" for g, _ in TEAMS])
def test_worker_kernel_exists_at_the_16_wave_cap(kds, g, bsm):
    name = _mangled("work", g, bsm)
    assert name in kds, f"{name} is not in {_ffi.LIB_PATH}"
    assert _vgprs(kds[name]) <= 128
