"""
The kernel set of the shipped library is what its launchers can reach, and it is pinned: the mangled kernel
names in elasticdeform_amd/libedhip.so -- the strings the host code hands to kernel registration, which sit in
the host library's .rodata -- are compared with tests/kernel_set.txt, one name per line, sorted.  Names only:
the device code is neither read nor searched.  No GPU is needed.

A change of the set is deliberate: regenerate the list with
    python tests/test_kernel_set.py > tests/kernel_set.txt
and say in the commit which kernels came or went and which launch site reaches the new ones
(profiles/kernel_set_audit.txt names the launch site of every class).
"""
import os
import re
import shutil
import struct
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "elasticdeform_amd", "libedhip.so")
LIST_PATH = os.path.join(ROOT, "tests", "kernel_set.txt")

# Classes no launcher of the shipped library can reach (docs/DESIGN_HISTORY.md, section I): a regenerated list
# must not bring them back.
#   deform_tile3_direct_kernel<T, ORDER, GRAD, WORKLIST>: order 0 is launched on every tile (WORKLIST false),
#   orders 1-5 as level 3 on a spill list (WORKLIST true), and neither the other way round;
#   deform_tile3_fwd_kernel<T, 0, ...>: order 0 has no source box;
#   wave_fwd_kernel / wave_grad_kernel<ORDER, ...>: the shipped rule sends orders 4 and 5 there.
UNREACHABLE = [
    r"deform_tile3_direct_kernelI[fd]Li0ELb[01]ELb1E",
    r"deform_tile3_direct_kernelI[fd]Li[1-5]ELb[01]ELb0E",
    r"deform_tile3_fwd_kernelI[fd]Li0E",
    r"wave_(fwd|grad)_kernelILi[1-3]E",
]


def registered_kernel_names(path):
    """The mangled names in the .rodata section of the host library, sorted."""
    blob = open(path, "rb").read()
    assert blob[:6] == b"\x7fELF\x02\x01", "not a little-endian ELF64 file"
    shoff, = struct.unpack_from("<Q", blob, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", blob, 0x3A)
    sections = [struct.unpack_from("<IIQQQQ", blob, shoff + i * shentsize) for i in range(shnum)]
    strtab = sections[shstrndx][4]
    for name_off, _type, _flags, _addr, offset, size in sections:
        start = strtab + name_off
        if blob[start:blob.index(b"\0", start)] == b".rodata":
            rodata = blob[offset:offset + size]
            break
    else:
        raise AssertionError("no .rodata section")
    names = re.findall(rb"(?:^|\x00)(_Z[A-Za-z0-9_$.]+)(?=\x00)", rodata)
    return sorted(set(n.decode() for n in names))


def _demangled(names):
    tool = shutil.which("c++filt")
    if not tool or not names:
        return names
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, timeout=30)
    lines = out.stdout.splitlines()
    return lines if out.returncode == 0 and len(lines) == len(names) else names


def test_kernel_set_is_the_committed_list():
    if not os.path.exists(LIB_PATH):
        pytest.skip("libedhip.so not built (run __graft_entry__.build())")
    built = registered_kernel_names(LIB_PATH)
    listed = open(LIST_PATH).read().split()
    assert listed == sorted(set(listed)), "tests/kernel_set.txt is not sorted or has duplicates"
    for pattern in UNREACHABLE:
        for where, names in (("the library", built), ("tests/kernel_set.txt", listed)):
            hits = [n for n in names if re.search(pattern, n)]
            assert not hits, "%s holds kernels no launcher can reach (%s):\n  %s" % (
                where, pattern, "\n  ".join(_demangled(hits)))
    added = sorted(set(built) - set(listed))
    removed = sorted(set(listed) - set(built))
    assert not added and not removed, (
        "the library's kernels are not those of tests/kernel_set.txt\n"
        "added (%d):\n  %s\nremoved (%d):\n  %s" % (len(added), "\n  ".join(_demangled(added)),
                                                    len(removed), "\n  ".join(_demangled(removed))))


if __name__ == "__main__":
    sys.stdout.write("".join(n + "\n" for n in registered_kernel_names(LIB_PATH)))
