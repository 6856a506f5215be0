#!/usr/bin/env python3
"""The HIP API calls of the last three placement calls of a rocprofv3 --hip-trace run, in order, per host thread:
    rocprofv3 --hip-trace -d DIR -- python tools/diag/place_once.py;  python tools/diag/api_sequence.py DIR
Two builds that make the same calls in the same order print the same text (diff the two outputs).

A host thread's share of a placement call begins with hipSetDevice (wepp_place_batch and each of its pool tasks select
the handle's device first), so a thread's trace is cut there; a piece with a kernel launch in it is a placement call --
the piece that ran place_device, all of it on that one thread.  The last three of them by start time are printed.  Which
thread ran a call is left out: wepp_place_batch hands a call's launches to whichever worker of its pool is free, so the
thread differs from run to run of one build.  A run of hipEventQuery / hipStreamQuery -- the host's poll, as long as the
device takes -- counts as one entry.  Meant for probes that place on one lane, like place_once.py: the pieces of a
pipelined call's two launch threads would be listed in the order they start, no more."""
import csv
import glob
import sys

POLL = ("hipEventQuery", "hipStreamQuery")
LAUNCH = ("hipLaunchKernel", "hipModuleLaunch", "hipExtModuleLaunch", "hipExtLaunchKernel")


def calls_of(trace_dir, last=3):
    rows = []
    for f in glob.glob(trace_dir + "/**/*hip_api_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            rows.append((int(r["Start_Timestamp"]), r["Thread_Id"], r["Function"]))
    rows.sort()
    pieces = {}                          # thread id -> its pieces [(start, [names])]
    for start, tid, name in rows:
        mine = pieces.setdefault(tid, [])
        if name == "hipSetDevice" or not mine:
            mine.append((start, []))
        names = mine[-1][1]
        if name in POLL:
            if not (names and names[-1] == "poll"):
                names.append("poll")
        else:
            names.append(name)
    placing = sorted((start, names) for ps in pieces.values() for start, names in ps if any(n.startswith(LAUNCH) for n in names))
    return placing[-last:]


if __name__ == "__main__":
    for k, (_, names) in enumerate(calls_of(sys.argv[1])):
        print("call %d of the last three, one host thread's, %d API calls:" % (k + 1, len(names)))
        for n in names:
            print("  " + n)
