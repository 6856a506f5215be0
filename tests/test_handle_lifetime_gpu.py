"""A handle destroyed while it holds everything it creates lazily (wepp_amd/csrc/handle.hpp: the members of wepp_mat
free what they own).  Three times over in one process: a handle is created; places a host batch of 65 536 reads in two
sub-batches (place_batch.cpp: the pipeline's streams and events, the pinned staging of reads and results, both lanes'
workspaces); places a small batch that is on the device; is given clade tables twice (the second replaces the first);
answers one wepp_epp_neighbors call (dfs_end joins the handle's blocks, the call's blocks are parked in its cache);
and is destroyed.  Then two handles live at once and go in the order they came.  Every call returns WEPP_OK (the
wrappers raise otherwise), the first and the last cycle place as the oracle does, and every handle reports the same
stats."""
import numpy as np
import pytest

import read_kinds as rk
import wepp_amd as w
from wepp_amd import _lib

pytestmark = pytest.mark.gpu
PIPELINED = 65_536             # read_check.hpp: BIG_BATCH_READS, from where set_pipeline's sub-batches are made
CYCLES = 3


def place_on_device(mat, reads):
    import torch
    dev = torch.device("cuda", mat.device)
    d_off = torch.from_numpy(reads.read_off.astype(np.int32)).to(dev)
    d_word = torch.from_numpy(reads.read_word.astype(np.int32)).to(dev)
    outs = [torch.zeros(reads.n_reads, dtype=torch.int32, device=dev) for _ in range(4)]
    mat.place_batch_device(d_off.data_ptr(), d_word.data_ptr(), reads.n_reads, int(reads.read_off[-1]), *[o.data_ptr() for o in outs], 0)
    torch.cuda.synchronize()
    a = [o.cpu().numpy() for o in outs]
    return w.PlacementResult(a[0].view(np.uint32), a[1], a[2].view(np.uint32), a[3].view(np.uint32))


def stats_of(mat):
    """every field of wepp_mat_stats, arrays as lists"""
    return {name: (list(v) if hasattr(v, "__len__") else v) for name, v in ((f[0], getattr(mat.stats, f[0])) for f in mat.stats._fields_)}


def destroy(mat):
    assert _lib.lib.wepp_mat_destroy(mat._h) == 0
    mat._h = None


def assert_oracle(res, want, idx, ctx):
    for name, got, exp in (("score", res.score, want["score"]), ("best_bfs_j", res.best_bfs_j, want["best_j"]),
                           ("num_best", res.num_best, want["num_best"]), ("has_unique", res.has_unique, want["has_unique"])):
        bad = np.flatnonzero(np.asarray(got) != np.asarray(exp)[idx])
        assert bad.size == 0, f"{ctx}: {name} differs at reads {bad[:10].tolist()}"


def test_handles_go_with_everything_they_hold(oracle):
    g = w.generate_tree(7, 3000, genome_len=2000, p_ambiguous=0.01, p_masked_node=0.002, root_mutations=2)
    few = g.reads(8, 256, read_len=150, amplicon_len=400, amplicon_step=300, p_substitution=0.004, p_n=0.01, p_iupac=0.1)
    want = oracle.OracleTree(g.tree).place_batch(few, nthreads=4)
    idx = np.resize(np.arange(few.n_reads), PIPELINED)
    many = rk.take(few, idx)
    n = g.tree.n_nodes
    clades = [(1 + np.arange(n, dtype=np.uint32) % 5).reshape(1, n), np.stack([np.arange(n, dtype=np.uint32) % 3, np.ones(n, np.uint32)])]
    piv = np.arange(0, n, 97, dtype=np.uint32)
    stats, first_nbr = [], None

    for cycle in range(CYCLES):
        mat = w.Mat(g.tree, device=0)
        stats.append(stats_of(mat))
        mat.set_pipeline(2)
        host = mat.place_batch(many)
        cls, _ = mat.last_plans(many.n_reads)          # (both sub-batches wrote their plan ids: the call was whole)
        assert cls.shape[0] == PIPELINED
        dev = place_on_device(mat, few)
        for cid in clades:
            mat.set_clades(cid, np.full(cid.shape[0], 9, np.uint32))
        nbr = mat.epp_neighbors(piv, 2, w.NBR_TO_PIVOT)
        if first_nbr is None:
            first_nbr = nbr
        for k in nbr:
            assert np.array_equal(nbr[k], first_nbr[k]), (cycle, k)
        if cycle in (0, CYCLES - 1):
            assert_oracle(host, want, idx, f"cycle {cycle}, host batch")
            assert_oracle(dev, want, np.arange(few.n_reads), f"cycle {cycle}, device batch")
        destroy(mat)

    a = w.Mat(g.tree, device=0)
    b = w.Mat(g.tree, device=0)
    stats += [stats_of(a), stats_of(b)]
    ra, rb = place_on_device(a, few), place_on_device(b, few)
    destroy(a)
    rb2 = b.place_batch(few)                           # (the handle that is left still works)
    destroy(b)
    for r, ctx in ((ra, "first of two"), (rb, "second of two"), (rb2, "second, the first gone")):
        assert_oracle(r, want, np.arange(few.n_reads), ctx)
    assert stats[0]["n_nodes"] == n and stats[0]["device_bytes"] > 0
    for i, s in enumerate(stats):
        assert s == stats[0], (i, {k: (s[k], stats[0][k]) for k in s if s[k] != stats[0][k]})
    g.close()
