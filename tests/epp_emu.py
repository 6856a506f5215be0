"""wepp_epp_assign, wepp_epp_resolve, wepp_epp_neighbors and wepp_epp_distances without a GPU: the entry points' own
host code (wepp_amd/csrc/{assign,resolve,neighbors}_capi.cpp, epp_host.cpp, errors.cpp) compiled by g++ against
tests/cxx/hip_emu -- the kernels as plain C++ with one host thread per lane, the HIP runtime as malloc / memcpy -- and
called through the structs of wepp_amd/_lib.py.  Every call gets a fresh handle over FlatView's arrays; afterwards
nothing may have been stored past what the call asked its device blocks for (emu_guard_check).

This checks the host sides' logic, buffer sizes and launch order and the kernels' logic and indexing.  It says
nothing about speed, occupancy, the device memory model or asynchrony between streams: those are the business of the
tests marked gpu."""
import atexit
import ctypes
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

import wepp_amd as w
from wepp_amd import _lib

_TESTS = os.path.dirname(os.path.abspath(__file__))
_CXX = os.path.join(_TESTS, "cxx")
_CSRC = os.path.join(os.path.dirname(_TESTS), "wepp_amd", "csrc")
_SOURCES = [os.path.join(_CXX, "epp_emu.cpp")] + [os.path.join(_CSRC, f) for f in (
    "assign_capi.cpp", "resolve_capi.cpp", "neighbors_capi.cpp", "epp_host.cpp", "errors.cpp")]
_P = lambda a: None if a is None else a.ctypes.data


@functools.lru_cache(maxsize=None)
def lib():
    """the emulated library, built once per session"""
    tmp = tempfile.mkdtemp(prefix="epp_emu_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    flags = ["g++", "-O1", "-std=c++17", "-fPIC", "-pthread", "-w", "-I", os.path.join(_CXX, "hip_emu")]
    objs = [os.path.join(tmp, os.path.basename(s) + ".o") for s in _SOURCES]
    jobs = [subprocess.Popen(flags + ["-c", s, "-o", o]) for s, o in zip(_SOURCES, objs)]
    assert all(j.wait() == 0 for j in jobs), "the emulated library does not compile"
    so = os.path.join(tmp, "libepp_emu.so")
    subprocess.check_call(flags + ["-shared"] + objs + ["-o", so])
    so = ctypes.CDLL(so)
    for name in ("wepp_epp_assign", "wepp_epp_resolve", "wepp_epp_neighbors", "wepp_epp_distances", "wepp_last_error"):
        getattr(so, name).restype, getattr(so, name).argtypes = _lib._SIGS[name]
    so.emu_mat_create.restype = ctypes.c_void_p
    so.emu_mat_create.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint32] * 2
    so.emu_mat_destroy.argtypes = so.emu_guard_check.argtypes = [ctypes.c_void_p]
    so.emu_res_chunk.restype = ctypes.c_uint32
    return so


def _call(tree, fn, *args):
    """fn(handle, *args) on a fresh handle over the tree; the code, or WeppError with the emulated library's message"""
    fv = w.FlatView(tree)
    woff, words, par = fv.get("node_woff"), fv.get("words"), fv.get("parent_dfs")
    words = words if words.size else np.zeros(1, np.uint32)
    max_pos = max(int(fv.get("maxnest").size), 1) - 1
    fv.close()
    h = lib().emu_mat_create(_P(woff), _P(words), _P(par), tree.n_nodes, max_pos)
    try:
        rc = fn(h, *args)
        assert lib().emu_guard_check(h) == 0, "a store outside what the call asked of device block %d" % (lib().emu_guard_check(h) - 1)
    finally:
        lib().emu_mat_destroy(h)
    return rc


def _finish(rc, out):
    """the outputs, or WeppError carrying them as .out (a short list buffer leaves every other output complete)"""
    if rc:
        err = w.WeppError(rc, lib().wepp_last_error().decode("utf-8", "replace"))
        err.out = out
        raise err
    return out


def _reads_c(reads):
    rw = reads.read_word if reads.read_word.size else np.zeros(1, np.uint32)
    return _lib.EppReadsC(reads.n_reads, _P(reads.read_off), _P(rw), _P(reads.start), _P(reads.end), _P(reads.degree)), rw


def assign(tree, reads, genome, sel, capacity=None):
    """capacity: entries of asg_sel (default: enough for every read to tie on the whole selection)"""
    R, K = reads.n_reads, len(sel)
    sel = np.ascontiguousarray(sel, np.uint32)
    cap = R * K if capacity is None else capacity
    md = np.zeros(R, np.int32); ne = np.zeros(R, np.uint32); off = np.full(R + 1, 77, np.uint64)
    asel = np.zeros(cap + 1, np.uint32); sr = np.full(K, 9, np.uint32); sd = np.full(K, 9, np.int64); sc = np.full(K, 9, np.uint32)
    cover = np.full((K, (genome + 31) // 32), 9, np.uint32)
    rd, keep = _reads_c(reads)
    o = _lib.AssignOutC(_P(md), _P(ne), _P(off), _P(asel), cap, _P(sr), _P(sd), _P(sc), _P(cover) if cover.size else None)
    rc = _call(tree, lib().wepp_epp_assign, ctypes.byref(rd), genome, K, _P(sel) if K else None, ctypes.byref(o))
    return _finish(rc, dict(min_dist=md, n_epp=ne, asg_off=off, asg_sel=asel[:int(off[R])] if rc == 0 else asel[:0],
                            sel_reads=sr, sel_degree=sd, sel_covered=sc, cover_bits=cover))


def resolve(tree, reads, genome, sel, residual, capacity=None):
    """residual as (pos, ref, mut); capacity: entries of rel_read (default: every read under every mutation)"""
    R, K = reads.n_reads, len(sel)
    sel = np.ascontiguousarray(sel, np.uint32)
    res = np.array([int(w.pack_read_word(p, r, m)) for p, r, m in residual], np.uint32)
    M = int(res.size)
    cap = R * M if capacity is None else capacity
    roff = np.full(M + 1, 77, np.uint64); rrel = np.zeros(cap + 1, np.uint32)
    ncov = np.full(max(M, 1), 9, np.uint32); nmask = np.full(max(M, 1), 9, np.uint32); bdeg = np.full(max(M, 1), 9, np.int64)
    bmask = np.full((max(M, 1), (K + 31) // 32), 9, np.uint32)
    hr = np.full((max(M, 1), K), 9, np.uint32); hd = np.full((max(M, 1), K), 9, np.int64); nt = np.full(1, 9, np.uint32)
    rd, keep = _reads_c(reads)
    o = _lib.ResolveOutC(_P(roff), _P(rrel), cap, _P(ncov), _P(nmask), _P(bdeg), _P(bmask), _P(hr), _P(hd), _P(nt))
    rc = _call(tree, lib().wepp_epp_resolve, ctypes.byref(rd), genome, K, _P(sel) if K else None, M, _P(res) if M else None,
               ctypes.byref(o))
    bits = np.unpackbits(bmask[:M].view(np.uint8), axis=1, bitorder="little")[:, :K]
    return _finish(rc, dict(rel_off=roff, rel_read=rrel[:int(roff[M])] if rc == 0 else rrel[:0], n_covered=ncov[:M], n_masked=nmask[:M],
                            best_degree=bdeg[:M], best_mask=bmask[:M], best=[np.flatnonzero(b).astype(np.uint32) for b in bits],
                            hap_reads=hr[:M], hap_degree=hd[:M], n_touched=int(nt[0])))


def neighbors(tree, piv, radius, form, skip=None, capacity=None):
    """capacity: entries of nbr_node / nbr_dist (default: every haplotype under every pivot)"""
    piv = np.ascontiguousarray(piv, np.uint32)
    N, K = tree.n_nodes, int(piv.size)
    sk = None if skip is None else np.ascontiguousarray(skip, np.uint8)
    cap = K * N if capacity is None else capacity
    off = np.full(K + 1, 77, np.uint64); node = np.zeros(cap + 1, np.uint32); nd = np.zeros(cap + 1, np.int32)
    top = np.full(max(K, 1), 9, np.uint32); nreg = np.full(max(K, 1), 9, np.uint32)
    o = _lib.NeighborsOutC(_P(off), _P(node), _P(nd), cap, _P(top), _P(nreg))
    rc = _call(tree, lib().wepp_epp_neighbors, K, _P(piv) if K else None, radius, form, _P(sk), ctypes.byref(o))
    n = int(off[K]) if rc == 0 else 0
    return _finish(rc, dict(nbr_off=off, nbr_node=node[:n], nbr_dist=nd[:n], top=top[:K], n_region=nreg[:K]))


def distances(tree, piv, form):
    piv = np.ascontiguousarray(piv, np.uint32)
    dist = np.zeros((int(piv.size), tree.n_nodes), np.int32)
    rc = _call(tree, lib().wepp_epp_distances, int(piv.size), _P(piv) if piv.size else None, form, _P(dist))
    return _finish(rc, dist)
