"""wepp_geno_diameters and wepp_geno_nearest without a GPU: geno_capi.cpp and errors.cpp compiled unchanged by g++
against tests/cxx/hip_emu, the kernels of geno_kernels.hip as plain C++ with one host thread per lane
(tests/cxx/geno_emu.cpp), in the manner of tests/epp_emu.py.  It checks the host side's logic, buffer sizes and
launch order and the kernels' logic and indexing; nothing about speed, occupancy or the device memory model."""
import atexit
import ctypes
import functools
import os
import shutil
import subprocess
import tempfile

import wepp_amd as w
from wepp_amd import _lib, geno

_TESTS = os.path.dirname(os.path.abspath(__file__))
_CXX = os.path.join(_TESTS, "cxx")
_CSRC = os.path.join(os.path.dirname(_TESTS), "wepp_amd", "csrc")
_SOURCES = [os.path.join(_CXX, "geno_emu.cpp"), os.path.join(_CSRC, "geno_capi.cpp"), os.path.join(_CSRC, "errors.cpp")]
_NAMES = ("wepp_geno_diameters", "wepp_geno_nearest", "wepp_geno_last_timing", "wepp_last_error")


@functools.lru_cache(maxsize=None)
def lib():
    """the emulated library, built once per session"""
    tmp = tempfile.mkdtemp(prefix="geno_emu_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    flags = ["g++", "-O1", "-std=c++17", "-fPIC", "-pthread", "-w", "-I", os.path.join(_CXX, "hip_emu"),
             "-include", os.path.join(_CXX, "geno_emu_extra.hpp")]
    objs = [os.path.join(tmp, os.path.basename(s) + ".o") for s in _SOURCES]
    jobs = [subprocess.Popen(flags + ["-x", "c++", "-c", s, "-o", o]) for s, o in zip(_SOURCES, objs)]
    assert all(j.wait() == 0 for j in jobs), "the emulated library does not compile"
    so = os.path.join(tmp, "libgeno_emu.so")
    subprocess.check_call(["g++", "-shared", "-pthread"] + objs + ["-o", so])
    so = ctypes.CDLL(so)
    for name in _NAMES:
        getattr(so, name).restype, getattr(so, name).argtypes = _lib._SIGS[name]
    return so


def _checked(fn):
    def call(*args):
        rc = fn(*args)
        if rc:
            raise w.WeppError(rc, lib().wepp_last_error().decode("utf-8", "replace"))
    return call


def diameters(item_off, item_word, grp_off, keep_bits=None, keep_positions=0):
    return geno.geno_diameters(item_off, item_word, grp_off, keep_bits, keep_positions, call=_checked(lib().wepp_geno_diameters))


def nearest(item_off, item_word, n_a, keep_bits=None, keep_positions=0, want_matrix=False):
    return geno.geno_nearest(item_off, item_word, n_a, keep_bits, keep_positions, want_matrix=want_matrix,
                             call=_checked(lib().wepp_geno_nearest))
