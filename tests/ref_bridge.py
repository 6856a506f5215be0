"""Builds and runs oracle/_ref/ref_driver: the REFERENCE's own mapper2_body and tree routines, compiled from where
the reference's sources lie, behind oracle/ref_driver.cpp.  Test infrastructure, like oracle_bridge.py.

What is compiled (flags of the reference's release build, CMakeLists.txt:14: -std=c++17 -O3 -DNDEBUG):
  * src/usher_mapper.cpp, unchanged;
  * two stretches of src/mutation_annotated_tree.cpp, written at build time into oracle/_ref/tree_part.cpp
    (git-ignored, never committed): everything before load_mutation_annotated_tree, and everything from the
    `/* === Node === */` marker to just before Tree::rotate_for_display.  The boundaries are found by these texts,
    never by line number, and the build fails if one is missing or if the assembled text names tbb::, boost:: or
    Parsimony::;
  * oracle/ref_driver.cpp, the serial driver (ours).
What is a stand-in: oracle/ref_shim/ -- the tbb containers as the std ones, a reader-writer lock that does nothing
(the driver is single-threaded), and empty headers for the other tbb / boost / protobuf names.  Not built: the
.pb / VCF loaders, the command line, WEPP's own cartesian_map and mutation_distance.

The reference's directory comes from WEPP_REFERENCE_DIR; where it does not exist build() returns None and builds
nothing (the committed fixtures under tests/golden/ hold what the binary recorded)."""
import json
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.environ.get("WEPP_REFERENCE_DIR", "/root/reference")
OUT_DIR = os.path.join(ROOT, "oracle", "_ref")
BIN = os.path.join(OUT_DIR, "ref_driver")
SHIM = os.path.join(ROOT, "oracle", "ref_shim")
DRIVER = os.path.join(ROOT, "oracle", "ref_driver.cpp")
FLAGS = ["-std=c++17", "-O3", "-DNDEBUG"]

FIRST_END = "Mutation_Annotated_Tree::Tree Mutation_Annotated_Tree::load_mutation_annotated_tree"
SECOND_BEGIN = "/* === Node === */"
SECOND_END = "void Mutation_Annotated_Tree::Tree::rotate_for_display"
FORBIDDEN = ("tbb::", "boost::", "Parsimony::")


def available():
    return os.path.isfile(os.path.join(REF_DIR, "src", "usher_mapper.cpp"))


def _find_once(text, what):
    at = [i for i in range(len(text)) if text.startswith(what, i) and (i == 0 or text[i - 1] == "\n")]
    if len(at) != 1:
        raise RuntimeError("reference tree source: %d lines begin with %r, expected one" % (len(at), what))
    return at[0]


def assemble_tree_part(text):
    """The two stretches of mutation_annotated_tree.cpp the scorer needs, as one translation unit."""
    a = _find_once(text, FIRST_END)
    b = _find_once(text, SECOND_BEGIN)
    c = _find_once(text, SECOND_END)
    if not (a < b < c):
        raise RuntimeError("reference tree source: the boundaries are not in the expected order")
    part = text[:a] + "\n" + text[b:c]
    for word in FORBIDDEN:
        if word in part:
            raise RuntimeError("reference tree source: the assembled part names %s" % word)
    return part


def _sources():
    src = os.path.join(REF_DIR, "src")
    deps = [os.path.join(src, f) for f in ("usher_mapper.cpp", "mutation_annotated_tree.cpp", "mutation_annotated_tree.hpp",
                                           "usher_graph.hpp", "Instrumentor.h")]
    deps += [DRIVER, os.path.abspath(__file__)]
    for d, _sub, files in os.walk(SHIM):
        deps += [os.path.join(d, f) for f in files]
    return src, deps


def build(force=False):
    """Returns the binary's path, or None where the reference's sources are not present."""
    if not available():
        return None
    src, deps = _sources()
    if not force and os.path.exists(BIN) and os.path.getmtime(BIN) >= max(os.path.getmtime(f) for f in deps):
        return BIN
    os.makedirs(OUT_DIR, exist_ok=True)
    with open(os.path.join(src, "mutation_annotated_tree.cpp")) as fh:
        part = assemble_tree_part(fh.read())
    tree_part = os.path.join(OUT_DIR, "tree_part.%d.cpp" % os.getpid())
    with open(tree_part, "w") as fh:
        fh.write(part)
    inc = ["-I", SHIM, "-I", src]
    objs = []
    jobs = []
    for name, path in (("usher_mapper", os.path.join(src, "usher_mapper.cpp")), ("tree_part", tree_part),
                       ("ref_driver", DRIVER)):
        obj = os.path.join(OUT_DIR, "%s.%d.o" % (name, os.getpid()))      # per process: two builds at once do not meet
        objs.append(obj)
        jobs.append(subprocess.Popen(["g++"] + FLAGS + inc + ["-c", path, "-o", obj]))
    tmp = BIN + ".tmp%d" % os.getpid()
    try:
        if any([j.wait() != 0 for j in jobs]):
            raise RuntimeError("the reference scorer did not compile")
        subprocess.check_call(["g++"] + FLAGS + objs + ["-o", tmp, "-lpthread"])
        os.replace(tree_part, os.path.join(OUT_DIR, "tree_part.cpp"))     # what was compiled, kept to be read
        os.replace(tmp, BIN)
    finally:
        for f in objs + [tmp, tree_part]:
            if os.path.exists(f):
                os.unlink(f)
    return BIN


def tree_lists(tree):
    n = tree.n_nodes
    par = tree.mut_par if tree.mut_par is not None else tree.mut_ref
    muts = []
    for i in range(n):
        lo, hi = int(tree.mut_off[i]), int(tree.mut_off[i + 1])
        muts.append([(int(tree.mut_pos[k]), int(tree.mut_ref[k]), int(par[k]), int(tree.mut_mut[k])) for k in range(lo, hi)])
    return [int(p) for p in tree.parent], muts


def encode(cases, mode):
    """cases: [(parent list, muts[node] = [(pos, ref, par, mut)], columns[c][node], samples)] as the driver's input"""
    out = ["WEPPREF 1 %s %d" % (mode, len(cases))]
    for parent, muts, columns, samples in cases:
        out.append("%d %d %d" % (len(parent), len(columns), len(samples)))
        for p, ml in zip(parent, muts):
            out.append(" ".join(["%d %d" % (p, len(ml))] + ["%d %d %d %d" % tuple(m) for m in ml]))
        for col in columns:
            for name in col:
                if any(ch.isspace() for ch in name):
                    raise ValueError("annotation with white space: %r" % name)
            out.append(" ".join("=" + name for name in col))
        for s in samples:
            out.append(" ".join(["%d" % len(s)] + ["%d %d %d %d" % (e[0], e[1], e[2], e[3] if len(e) > 3 else 0) for e in s]))
    return "\n".join(out) + "\n"


def run(cases, mode="full"):
    """One process of the driver over cases (see encode): a list of {"bfs": ..., "results": ...} per case."""
    exe = build()
    if exe is None:
        raise RuntimeError("the reference's sources are not at %s" % REF_DIR)
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as fh:
        fh.write(encode(cases, mode))
        path = fh.name
    try:
        done = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=False)
    finally:
        os.unlink(path)
    if done.returncode != 0:
        raise RuntimeError("ref_driver failed (%d): %s" % (done.returncode, done.stderr.decode()[-500:]))
    lines = done.stdout.decode().splitlines()
    if len(lines) != len(cases):
        raise RuntimeError("ref_driver wrote %d lines for %d cases" % (len(lines), len(cases)))
    return [json.loads(ln) for ln in lines]
