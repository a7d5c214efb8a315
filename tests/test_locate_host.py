"""CPU checks of the batched-locate boundary (no kernel is launched): the four calls are
declared and exported, bad arguments are refused with a message before any device call, and
the C++ mirror (sas::SaNaive::locate / search_between) compiles warning-free and links."""
import ctypes as C
import errno
import os
import subprocess

import numpy as np

from sas_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sas_locate_offsets", "sas_locate_fill", "sas_locate", "sas_locate_fixed")
DEV = _lib.SAS_DEVICE_PTRS


def test_symbols_declared_and_exported():
    declared = _lib.declared_symbols()
    L = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in declared and hasattr(L, name), name
    assert _lib.SAS_LOCATE_U32 & (_lib.SAS_LOCATE_U32 - 1) == 0
    # the flag shares no bit with the other search-call flags
    others = (_lib.SAS_DEVICE_PTRS | _lib.SAS_NO_LDS_TOP | _lib.SAS_VALIDATE | _lib.SAS_PREFIX_RANGE |
              _lib.SAS_NO_PREFIX_TABLE | _lib.SAS_ROUTE_PACKED | _lib.SAS_RANGE_NO_INLINE |
              _lib.SAS_QUERIES_ARE_SLICES | _lib.SAS_LOCATE_NO_PARTITION)
    assert _lib.SAS_LOCATE_U32 & others == 0


def fake_index(n: int):
    """Zeroed stand-in for a sas_index whose first field, the text length, is n: enough for
    the argument checks, which read nothing else before they refuse."""
    buf = (C.c_uint64 * 1024)()
    buf[0] = n
    return buf


def test_fake_index_layout_is_pinned(tmp_path):
    """fake_index puts n at offset 0: the library's own header must agree, or the argument
    checks below would read garbage (a host-only syntax check of csrc/common.hpp)."""
    src = tmp_path / "layout.hip"
    src.write_text('#include "common.hpp"\n#include <cstddef>\n'
                   'static_assert(offsetof(sas_index, n) == 0, "sas_index::n must stay the first field");\n'
                   'static_assert(sizeof(sas_index) <= 1024 * 8, "fake_index is 8 KiB");\n')
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-std=c++17", "--offload-host-only", "-fsyntax-only", "-Wno-unused-command-line-argument",
                           "-I", os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc"), str(src)])


def einval(L, rc, word: bytes):
    assert rc == errno.EINVAL, rc
    assert word in L.sas_last_error(), L.sas_last_error()


def test_null_and_host_pointers_refused_before_any_device_call():
    L = _lib.lib()
    x = fake_index(1000)
    a = np.zeros(8, np.uint64)
    p = a.ctypes.data
    # null arguments
    einval(L, L.sas_locate_offsets(None, p, p, 4, 0, p, None, DEV), b"sas_locate_offsets: null")
    einval(L, L.sas_locate_offsets(x, p, p, 4, 0, None, None, DEV), b"sas_locate_offsets: null")
    einval(L, L.sas_locate_offsets(x, None, p, 4, 0, p, None, DEV), b"sas_locate_offsets: null")
    einval(L, L.sas_locate_fill(None, p, p, 4, p, 8, None, DEV), b"sas_locate_fill: null")
    einval(L, L.sas_locate_fill(x, p, None, 4, p, 8, None, DEV), b"sas_locate_fill: null")
    einval(L, L.sas_locate_fill(x, p, p, 4, None, 8, None, DEV), b"sas_locate_fill: null")
    einval(L, L.sas_locate(None, p, p, p, 1, 0, p, p, 8, None, None, 0), b"sas_locate: null")
    einval(L, L.sas_locate(x, p, None, p, 1, 0, p, p, 8, None, None, 0), b"sas_locate: null")
    einval(L, L.sas_locate(x, p, p, p, 1, 0, None, p, 8, None, None, 0), b"sas_locate: null")
    einval(L, L.sas_locate(x, p, p, p, 1, 0, p, None, 8, None, None, 0), b"sas_locate: null")
    einval(L, L.sas_locate_fixed(x, None, 4, 1, 0, p, p, 8, None, None, 0), b"sas_locate_fixed: null")
    einval(L, L.sas_locate_fixed(x, p, 4, 1, 0, None, p, 8, None, None, 0), b"sas_locate_fixed: null")
    # host pointers to the device-only calls
    einval(L, L.sas_locate_offsets(x, p, p, 4, 0, p, None, 0), b"device pointers only")
    einval(L, L.sas_locate_fill(x, p, p, 4, p, 8, None, 0), b"device pointers only")


def test_u32_positions_refused_for_a_text_of_2_32_chars():
    L = _lib.lib()
    a = np.zeros(8, np.uint64)
    p = a.ctypes.data
    U32 = _lib.SAS_LOCATE_U32
    for n in (1 << 32, 1 << 34):
        x = fake_index(n)
        einval(L, L.sas_locate_fill(x, p, p, 4, p, 8, None, DEV | U32), b"SAS_LOCATE_U32")
        einval(L, L.sas_locate(x, p, p, p, 1, 0, p, p, 8, None, None, U32), b"SAS_LOCATE_U32")
        einval(L, L.sas_locate(x, p, p, p, 1, 0, p, p, 8, None, None, DEV | U32), b"SAS_LOCATE_U32")
        einval(L, L.sas_locate_fixed(x, p, 4, 1, 0, p, p, 8, None, None, U32), b"SAS_LOCATE_U32")


CPP = r"""
#include "sas.hpp"
int main(int argc, char**) {
    std::vector<uint8_t> t = sas::random_string(1000);
    if (argc < 100) return 0;  // linked, not run: no GPU here
    sas::SaNaive idx = sas::SaNaive::build(t);
    const sas::Seq s(t);
    const sas::SaNaive::Located r = idx.locate({s.slice(0, 3), s.slice(5, 5), s.slice(10, 40)}, 7);
    const std::vector<size_t> v = idx.search_between(s.slice(0, 2), s.slice(3, 9));
    return (int)(r.off.size() + r.pos.size() + v.size());
}
"""


def test_cpp_locate_compiles_and_links(tmp_path):
    src = tmp_path / "locate.cpp"
    src.write_text(CPP)
    inc = os.path.join(REPO, "include")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", inc, str(src)])
    exe = tmp_path / "locate"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", inc, str(src), "-o", str(exe),
                           "-L", libdir, "-lsas_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"])
    assert os.access(exe, os.X_OK)
