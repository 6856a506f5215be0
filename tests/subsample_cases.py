"""The inputs the subsampling tests share (test_subsample_model.py checks on the CPU that each of them meets the
condition the GPU comparison rests on; test_sam_subsample_gpu.py runs them), and their model answers, computed once.

The layout units of the device code the shapes are chosen by (wepp_amd/csrc/sam_subsample.hpp): B = 8 trials per batch
of the trial pile-up, tiles of 256 sites, chunks of 512 entries of a tile's read list, 4096 reads per workgroup of the
radix select's histogram."""
import functools
import random

import sam_model as sm
import subsample_model as sub

BATCH, TILE, CHUNK, SELECT_CHUNK = 8, 256, 512, 4096
AF = sm.stof("0.005")


def tiled_reads(seed, G, n):
    """reads of 1 .. 40 columns on G sites, a few variants drawn many times; every boundary between tiles of 256 sites is
    straddled, one read starts at site 1, one ends at the last site, one ends right before and one starts right at each
    boundary"""
    rng = random.Random(seed)
    ref = sm.random_reference(rng, G)
    windows = [(0, min(G, 9)), (G - min(G, 7), min(G, 7))]
    for b in range(TILE, G, TILE):
        windows += [(b - 5, min(11, G - b + 5)), (b - 3, 3), (b, min(4, G - b))]
    while len(windows) < 12:
        length = rng.randint(1, min(40, G))
        windows.append((rng.randint(0, G - length), length))
    variants = []
    for start, length in windows:
        for _ in range(2):
            s = list(ref[start:start + length])
            for j in range(length):
                if rng.random() < 0.1:
                    s[j] = rng.choice("ACGTN_")
            variants.append((start, "".join(s)))
    picks = list(range(len(variants))) + [rng.randrange(len(variants)) for _ in range(n - len(variants))]
    rng.shuffle(picks)
    return ref, [(f"r{i}", *variants[k]) for i, k in enumerate(picks)]


def short_reads(seed, G, n):
    """n reads of 1 .. 3 columns"""
    rng = random.Random(seed)
    ref = sm.random_reference(rng, G)
    reads = []
    for i in range(n):
        length = rng.randint(1, 3)
        start = rng.randint(0, G - length)
        s = "".join(c if rng.random() > 0.2 else rng.choice("ACGTN_") for c in ref[start:start + length])
        reads.append((f"r{i}", start, s))
    return ref, reads


def floors():
    """39 reads over sites 1 .. 20 and: twelve reads each alone on two sites of its own (no trial can keep them all: sites
    of the full table that no kept read covers); site 41 with many N columns and two A (kept reads cover it with N
    only); reads made of N and _ only"""
    rng = random.Random(3)
    ref = sm.random_reference(rng, 128)
    reads = [(f"a{i}", 0, ref[0:20] if i % 4 else ref[0:10] + "N" + ref[11:20]) for i in range(39)]
    reads += [(f"lonely{i}", 64 + 3 * i, ref[64 + 3 * i:66 + 3 * i]) for i in range(12)]
    reads += [(f"n{i}", 40, "N") for i in range(30)] + [("x0", 40, "A"), ("x1", 40, "A")]
    reads += [(f"g{i}", 50, "N_N_") for i in range(6)] + [("h", 56, "NN")]
    rng.shuffle(reads)
    return ref, reads


def deep():
    """70 000 equal one-column reads at one site and 300 ordinary reads"""
    ref, reads = sm.gen_aligned(21, G=200, n_reads=300)
    reads = reads + [(f"d{i}", 77, ref[77]) for i in range(70000)]
    random.Random(4).shuffle(reads)
    return ref, reads


def identical():
    ref = sm.random_reference(random.Random(9), 64)
    return ref, [(f"r{i}", 5, ref[5:20] + "N_") for i in range(50)]


def _cases():
    c = {}
    ref, reads = sm.gen_aligned(11, G=200, n_reads=300)
    for m in (1, 299, 63, 64, 65, 255, 256, 257):                      # subset sizes
        c[f"m{m}"] = (ref, reads, AF, 3, 100 + m, m, 12)
    ref, reads = sm.gen_aligned(12, G=200, n_reads=130)
    for T in (1, BATCH - 1, BATCH, BATCH + 1, 2 * BATCH + 1):         # trials around the batch
        c[f"T{T}"] = (ref, reads, AF, 3, 200 + T, 64, T)
    for G in (TILE - 1, TILE, TILE + 1, 2 * TILE + 5):                # genome sizes around the tile
        ref, reads = tiled_reads(G, G, 180)
        c[f"G{G}"] = (ref, reads, AF, 3, 300 + G, 90, 10)
    for n in (CHUNK - 1, CHUNK, CHUNK + 1):                           # one tile whose list is a chunk -1, +0, +1
        ref, reads = sm.gen_aligned(40 + n, G=100, n_reads=n)
        c[f"n{n}"] = (ref, reads, AF, 3, 400 + n, n // 2, 9)
    for n in (SELECT_CHUNK - 1, SELECT_CHUNK, SELECT_CHUNK + 1):      # the histogram's chunk of reads
        ref, reads = short_reads(n, 300, n)
        c[f"n{n}"] = (ref, reads, AF, 3, 500 + n, 2000, 3)
    c["floors"] = (*floors(), AF, 3, 9, 40, 3)                        # (a seed under which the winner shows all three)
    c["deep"] = (*deep(), AF, 3, 5, 66000, 2)
    c["ties"] = (*identical(), AF, 3, 6, 20, 9)
    ref, reads = sm.gen_aligned(13, G=200, n_reads=130)
    c["passes"] = (ref, reads, AF, 3, 7, 64, 20)
    deepest = max(sum(row) for row in sm.frequency_table(reads, len(ref)))
    c["full_table"] = (ref, reads, 0.02, deepest - 5, 8, 64, 5)       # min_depth that only the full table's deepest sites reach
    return c


CASES = _cases()


@functools.lru_cache(maxsize=None)
def model(name):
    ref, reads, min_af, min_depth, seed, m, T = CASES[name]
    return sub.subsample(ref, reads, min_af, min_depth, seed, m, T)
