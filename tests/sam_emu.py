"""wepp_sam_build and wepp_sam_build_subsampled without a GPU: sam_capi.cpp, sam_subsample_capi.cpp and errors.cpp
compiled unchanged by g++ against tests/cxx/hip_emu, the kernels of sam_kernels.hip and sam_subsample_kernels.hip as
plain C++ with one host thread per lane, in the manner of tests/geno_emu.py; rocPRIM's scan and merge sort are serial
stand-ins.  It checks the host sides' logic, buffer sizes and launch order and the kernels' logic and indexing; nothing
about speed, occupancy, LDS limits or the device memory model, and the divergence's logarithm is the host's."""
import atexit
import ctypes
import functools
import os
import shutil
import subprocess
import tempfile

import wepp_amd as w
from wepp_amd import _lib

_TESTS = os.path.dirname(os.path.abspath(__file__))
_CXX = os.path.join(_TESTS, "cxx")
_CSRC = os.path.join(os.path.dirname(_TESTS), "wepp_amd", "csrc")
_SOURCES = [os.path.join(_CXX, "sam_emu.cpp")] + [os.path.join(_CSRC, f) for f in (
    "sam_subsample_kernels.hip", "sam_capi.cpp", "sam_subsample_capi.cpp", "errors.cpp")]
_NAMES = ("wepp_sam_build", "wepp_sam_fetch_words", "wepp_sam_last_timing", "wepp_sam_build_subsampled", "wepp_sam_subsample_last_timing",
          "wepp_last_error")


@functools.lru_cache(maxsize=None)
def lib():
    """the emulated library, built once per session"""
    tmp = tempfile.mkdtemp(prefix="sam_emu_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    flags = ["g++", "-O1", "-std=c++17", "-fPIC", "-pthread", "-w", "-ffp-contract=off", "-I", os.path.join(_CXX, "sam_emu"),
             "-I", os.path.join(_CXX, "hip_emu"), "-include", os.path.join(_CXX, "sam_emu_extra.hpp")]
    objs = [os.path.join(tmp, os.path.basename(s) + ".o") for s in _SOURCES]
    jobs = [subprocess.Popen(flags + ["-x", "c++", "-c", s, "-o", o]) for s, o in zip(_SOURCES, objs)]
    assert all(j.wait() == 0 for j in jobs), "the emulated library does not compile"
    so = os.path.join(tmp, "libsam_emu.so")
    subprocess.check_call(["g++", "-shared", "-pthread"] + objs + ["-o", so])
    so = ctypes.CDLL(so)
    for name in _NAMES:
        getattr(so, name).restype, getattr(so, name).argtypes = _lib._SIGS[name]
    return so


def sam_build(*args, **kw):
    return w.sam_build(*args, so=lib(), **kw)


def sam_build_subsampled(*args, **kw):
    return w.sam_build_subsampled(*args, so=lib(), **kw)
