"""The pass-2 kernels (pass2_kernels.hip: k_scores<false>, k_scores<true>, k_imputed, k_excess) at their chunk,
checkpoint, block and path edges: every call of every case of tests/pass2_cases.py through the public API against the
oracle, every element of every output, exactly.  tests/test_pass2_cases.py shows on the input's side that each case
sits on its edge.  Every call is made twice on the same handle -- the handle's grow-only block is reused, the cursors
must be cleared -- and the two results are identical byte for byte; the handles print what they launch
(WEPP_DEBUG_PLANS=1: the `[scores]` and `[best_nodes]` lines), which must be what the restated rule predicts."""
import numpy as np
import pytest

import pass2_cases as pc
import wepp_amd as w
from wepp_amd.api import _ptr

pytestmark = pytest.mark.gpu
WEPP_ELIMIT = 4


_of_kind = pc.of_kind


def test_every_case_runs_here():
    assert sorted(n for k in ("scores", "best", "imputed", "excess") for n in _of_kind(k)) == sorted(pc.CASES)


@pytest.fixture
def mat_of(monkeypatch):
    """Handles that print their launches; closed when the test ends."""
    monkeypatch.setenv("WEPP_DEBUG_PLANS", "1")
    made = []

    def make(tree):
        made.append(w.Mat(tree))
        return made[-1]
    yield make
    for m in made:
        m.close()


@pytest.mark.parametrize("name", _of_kind("scores"))
def test_per_node_scores(oracle, mat_of, capfd, name):
    c = pc.CASES[name]()
    mat = mat_of(c.tree)
    for i, b in enumerate(c.calls):
        capfd.readouterr()
        first = mat.place_batch(b.reads, per_node_scores=True).per_node_scores
        launched, _ = pc.parse_debug_lines(capfd.readouterr().err)
        assert launched == [(b.n_reads,) + c.chunks(b.n_reads)], (name, i)
        second = mat.place_batch(b.reads, per_node_scores=True).per_node_scores
        assert first.tobytes() == second.tobytes(), (name, i)
        want = pc.want_scores(name, i)[b.index]
        assert first.shape == want.shape and first.dtype == np.int32
        bad = np.argwhere(first != want)
        assert bad.size == 0, (name, i, len(bad), bad[:5].tolist())


def _stream_of(flat, kind, index):
    """The stream of the flat image a `[best_nodes]` line names."""
    return "w%d" % index if kind == "window" else None if index == flat.n_streams - 1 else index


@pytest.mark.parametrize("name", _of_kind("best"))
def test_best_nodes(oracle, mat_of, capfd, name):
    c = pc.CASES[name]()
    flat = c.info.flat
    mat = mat_of(c.tree)
    for i, (b, crowns) in enumerate(c.calls):
        ctx = (name, i)
        want = pc.want_best(name, i)
        mat.set_use_crowns(crowns)
        res = mat.place_batch(b.reads)
        assert res.score.tolist() == [want[q][0] for q in b.index], ctx
        assert res.num_best.tolist() == [want[q][1] for q in b.index], ctx
        capfd.readouterr()
        off, nodes = mat.best_nodes_csr(b.reads, res)
        _, plans = pc.parse_debug_lines(capfd.readouterr().err)
        off2, nodes2 = mat.best_nodes_csr(b.reads, res)
        assert off.tobytes() == off2.tobytes() and nodes.tobytes() == nodes2.tobytes(), ctx
        assert off.tolist() == np.concatenate([[0], np.cumsum([want[q][1] for q in b.index])]).tolist(), ctx
        assert nodes.dtype == np.uint32 and nodes.tolist() == np.concatenate([want[q][2] for q in b.index]).tolist(), ctx
        # what was launched: every plan's chunks by the rule, over that plan's stream and its count of reads
        assert sum(p[2] for p in plans) == b.n_reads and len(set(p[:2] for p in plans)) == len(plans), (ctx, plans)
        for kind, index, count, nchunks, bpc in plans:
            assert (nchunks, bpc) == c.chunks(count, _stream_of(flat, kind, index)), (ctx, kind, index, count)
        if not crowns:
            assert [p[:3] for p in plans] == [("stream", flat.n_streams - 1, b.n_reads)], (ctx, plans)
        if crowns and name == "many_reads_few_ties":
            assert len(plans) >= 3 and all(count < b.n_reads for _, _, count, _, _ in plans), plans      # strict subsets
        if crowns and name == "plans_mixed":
            kinds = [p[0] for p in plans]
            assert len(plans) >= 3 and "window" in kinds and ("stream", flat.n_streams - 1) in [p[:2] for p in plans], plans


@pytest.mark.parametrize("name", _of_kind("imputed"))
def test_imputed_mutations(oracle, mat_of, name):
    c = pc.CASES[name]()
    mat = mat_of(c.tree)
    for i, (b, bj) in enumerate(c.calls):
        first = mat.imputed_mutations(b.reads, bj)
        second = mat.imputed_mutations(b.reads, bj)
        want = pc.want_imputed(name, i)
        assert first == second, (name, i)
        assert first == want, (name, i, [q for q in range(len(want)) if first[q] != want[q]][:5])


@pytest.mark.parametrize("name", _of_kind("excess"))
def test_excess_mutations(oracle, mat_of, name):
    c = pc.CASES[name]()
    mat = mat_of(c.tree)
    for i, (b, pr, pj) in enumerate(c.calls):
        first = mat.excess_mutations(b.reads, pr, pj)
        second = mat.excess_mutations(b.reads, pr, pj)
        want = pc.want_excess(name, i)
        assert first == second, (name, i)
        assert first == want, (name, i, [q for q in range(len(want)) if first[q] != want[q]][:5])


def test_error_paths_next_to_the_edges(oracle, mat_of):
    """A node index of N is rejected; a capacity one short is WEPP_ELIMIT with the size needed, the offsets filled."""
    lib = w._lib.lib
    last_error = lambda: lib.wepp_last_error().decode()
    # imputed: the call of exactly 256 pairs
    c = pc.CASES["pairs_256"]()
    n = c.tree.n_nodes
    mat = mat_of(c.tree)
    b, bj = c.calls[1]
    bad = bj.copy()
    bad[-1] = n
    with pytest.raises(w.WeppError, match="best_bfs_j out of range"):
        mat.imputed_mutations(b.reads, bad)
    per = [len(pc.ambiguous_entries(b.lists[q])) for q in b.index]
    total = sum(per)
    off = np.full(b.n_reads + 1, 0xFFFFFFFF, np.uint32)
    pos, nuc = np.zeros(total, np.int32), np.zeros(total, np.uint8)
    rc = lib.wepp_imputed_mutations(mat._h, _ptr(b.reads.read_off), _ptr(b.reads.read_word), b.n_reads, _ptr(bj), _ptr(off), _ptr(pos), _ptr(nuc), total - 1)
    assert rc == WEPP_ELIMIT and "need %d" % total in last_error() and off.tolist() == np.concatenate([[0], np.cumsum(per)]).tolist()
    assert mat.imputed_mutations(b.reads, bj) == pc.want_imputed("pairs_256", 1)
    # excess: the call of exactly 128 pairs
    c = pc.CASES["pairs_128"]()
    n = c.tree.n_nodes
    mat = mat_of(c.tree)
    b, pr, pj = c.calls[1]
    bad = pj.copy()
    bad[0] = n
    with pytest.raises(w.WeppError, match="pair_bfs_j out of range"):
        mat.excess_mutations(b.reads, pr, bad)
    want = pc.want_excess("pairs_128", 1)
    total = sum(len(x) for x in want)
    off = np.full(len(pr) + 1, 1 << 63, np.uint64)
    out = [np.zeros(total, np.int32)] + [np.zeros(total, np.uint8) for _ in range(3)]
    rc = lib.wepp_excess_mutations(mat._h, _ptr(b.reads.read_off), _ptr(b.reads.read_word), b.n_reads, len(pr), _ptr(pr), _ptr(pj),
                                   _ptr(off), *[_ptr(a) for a in out], total - 1)
    assert rc == WEPP_ELIMIT and "need %d" % total in last_error() and off.tolist() == np.concatenate([[0], np.cumsum([len(x) for x in want])]).tolist()
    assert mat.excess_mutations(b.reads, pr, pj) == want
    # best nodes: the star's three reads
    c = pc.CASES["ties_span_chunks"]()
    mat = mat_of(c.tree)
    b, _ = c.calls[0]
    res = mat.place_batch(b.reads)
    total = int(res.num_best.sum())
    assert total == sum(x[1] for x in pc.want_best("ties_span_chunks", 0))
    off = np.full(b.n_reads + 1, 1 << 63, np.uint64)
    nodes = np.zeros(total, np.uint32)
    rc = lib.wepp_best_nodes(mat._h, _ptr(b.reads.read_off), _ptr(b.reads.read_word), b.n_reads, _ptr(res.score), _ptr(res.num_best),
                             _ptr(off), _ptr(nodes), total - 1)
    assert rc == WEPP_ELIMIT and "need %d" % total in last_error() and off.tolist() == np.concatenate([[0], np.cumsum(res.num_best)]).tolist()
    assert not nodes.any()
