"""host side of the timed steps from a rocprofv3 --hip-trace: the wait for the routing counters, and from its return to the next kernel launch.
A device call is found by its FIRST kernel launch (k_route's: the first launch behind a gap in the launches, i.e. behind
the wait).  With the counters' copy the wait shows as a run of hipEventQuery / hipStreamQuery; with k_step's report the
host polls memory and makes no API call while it waits: the wait is then the gap between the call's last API call in
front of it (k_step's launch, or the blind k_scatter's) and the first one behind it."""
import csv, glob, sys, statistics as st
rows = []
for f in glob.glob(sys.argv[1] + "/**/*hip_api_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Function"], r.get("Thread_Id", "")))
rows.sort()
POLL = ("hipEventQuery", "hipStreamQuery")
LAUNCH = ("hipLaunchKernel", "hipModuleLaunch", "hipExtModuleLaunch", "hipExtLaunchKernel")
is_launch = lambda name: name.startswith(LAUNCH)
polls = []          # (first start, last end, n, index behind)
i = 0
while i < len(rows):
    if rows[i][2] in POLL:
        j = i
        while j + 1 < len(rows) and rows[j + 1][2] in POLL:
            j += 1
        polls.append((rows[i][0], rows[j][1], j - i + 1, j + 1))
        i = j + 1
    else:
        i += 1
launches = [k for k, r in enumerate(rows) if is_launch(r[2])]
if len(polls) < 16:
    # no queries: the steps by their launches.  The timed loop is the end of the run: two launches a step (k_route, k_step).
    per_call = 2
    firsts = launches[-per_call * 16::per_call]
    calls_api, wait, period, tail = [], [], [], []
    for a, b in zip(firsts[:-1], firsts[1:]):
        seq = rows[a:b]
        calls_api.append(len(seq))
        # the wait: the longest silence between two API calls of the step
        gaps = [(seq[k + 1][0] - seq[k][1], k) for k in range(len(seq) - 1)] + [(rows[b][0] - seq[-1][1], len(seq) - 1)]
        g, k = max(gaps)
        wait.append(g / 1e3)
        tail.append((rows[b][0] - (seq[k][1] + g)) / 1e3)
        period.append((rows[b][0] - rows[a][0]) / 1e3)
    print("no run of queries: steps by their launches;", len(period), "steps, API calls per device call:", sorted(set(calls_api)))
    print("longest silence of a step (the poll of memory): mean %.1f min %.1f max %.1f us" % (st.mean(wait), min(wait), max(wait)))
    print("end of that silence to the start of the next k_route launch call: mean %.1f min %.1f max %.1f us" % (st.mean(tail), min(tail), max(tail)))
    print("k_route launch call to k_route launch call (the host's step): mean %.1f min %.1f max %.1f us" % (st.mean(period), min(period), max(period)))
    names = {}
    for a, b in zip(firsts[:-1], firsts[1:]):
        s = tuple(r[2] for r in rows[a:b])
        names[s] = names.get(s, 0) + 1
    for seq, n in sorted(names.items(), key=lambda x: -x[1])[:3]:
        print(n, "x API calls of a step:", " ".join(seq))
    sys.exit(0)
polls = polls[-16:-1]
wait, tail, calls, period, names, per_call = [], [], [], [], {}, []
for k, (a, b, n, nxt) in enumerate(polls):
    wait.append((b - a) / 1e3)
    m = nxt
    seq = []
    while m < len(rows) and not is_launch(rows[m][2]):
        seq.append(rows[m][2])
        m += 1
    if m < len(rows):
        tail.append((rows[m][0] - b) / 1e3)
        calls.append(len(seq))
        names[tuple(seq)] = names.get(tuple(seq), 0) + 1
    if k + 1 < len(polls):
        period.append((polls[k + 1][1] - b) / 1e3)
        per_call.append(polls[k + 1][3] - nxt)
print("polls", len(polls), "queries per poll: mean %.0f" % st.mean(p[2] for p in polls), "API calls per device call:", sorted(set(per_call)))
print("poll, first query to its return: mean %.1f min %.1f max %.1f us" % (st.mean(wait), min(wait), max(wait)))
print("return of the poll to the start of the next kernel launch call: mean %.1f min %.1f max %.1f us, API calls in between: %s" % (st.mean(tail), min(tail), max(tail), sorted(set(calls))))
print("poll return to poll return (the host's step): mean %.1f min %.1f max %.1f us" % (st.mean(period), min(period), max(period)))
for seq, n in sorted(names.items(), key=lambda x: -x[1])[:3]:
    print(n, "x between poll and launch:", " ".join(seq))
