#!/usr/bin/env python3
"""Run by tests/test_route_tables_gpu.py::test_saturated_length_fields in a CHILD process with WEPP_PLACE_LIB pointing at
a variant build of the library (tools/build_variant.sh rtlen3 -DWEPP_RT_LEN_BITS=3: the library is chosen when the
package is imported): places the reads of <in.npz> on the test's tree, into arrays pre-filled with 0x7FFFFFFF, and
writes the four arrays to <out.npz>.  Prints one JSON line with the build's length-field width."""
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import test_route_tables_gpu as T  # noqa: E402
import wepp_amd as w  # noqa: E402
from wepp_amd import _lib  # noqa: E402


def main():
    src = np.load(sys.argv[1])
    reads = w.Reads(src["read_off"], src["read_word"])
    fn = _lib.lib.wepp_debug_route_len_bits
    fn.restype, fn.argtypes = ctypes.c_uint32, []
    g = T.make_tree()
    mat = w.Mat(g.tree)
    try:
        res = T.place_filled(mat, reads)
    finally:
        mat.close()
    np.savez(sys.argv[2], best_bfs_j=res.best_bfs_j, score=res.score, num_best=res.num_best, flags=res.flags)
    print(json.dumps({"len_bits": int(fn()), "reads": reads.n_reads}), flush=True)


if __name__ == "__main__":
    main()
