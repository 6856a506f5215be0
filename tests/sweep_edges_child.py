"""Child process of tests/test_sweep_edges_gpu.py: places the cases of one group of tests/sweep_cases.py with
WEPP_DEBUG_PLANS=1 in the environment.  stderr carries the library's `[plan]` lines between `[case] <name> <count>`
markers, stdout one JSON line per placed batch: the four result arrays and the per-read plan ids."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import sweep_cases as sc  # noqa: E402
import wepp_amd as w  # noqa: E402


def main(names):
    for name in names:
        case = sc.CASES[name]()
        mat = w.Mat(case.tree)
        sc.apply_knobs(mat, case.knobs)
        for count in case.counts:
            reads = case.reads.slice(0, count)
            os.write(2, ("[case] %s %d\n" % (name, count)).encode())
            res = mat.place_batch(reads)
            pcls, pst = mat.last_plans(count)
            win, crown = mat.last_crowns(count)
            print(json.dumps(dict(name=name, count=count, score=res.score.tolist(), best_bfs_j=res.best_bfs_j.tolist(),
                                  num_best=res.num_best.tolist(), flags=res.flags.tolist(), pcls=pcls.tolist(),
                                  pst=pst.tolist(), win=np.asarray(win).tolist(), crown=np.asarray(crown).tolist())), flush=True)
        mat.close()


if __name__ == "__main__":
    main(sys.argv[1:])
