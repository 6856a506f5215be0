"""host side of the timed steps from a rocprofv3 --hip-trace: the poll for the routing counters, and from its return to the next kernel launch"""
import csv, glob, sys, statistics as st
rows = []
for f in glob.glob(sys.argv[1] + "/**/*hip_api_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Function"], r.get("Thread_Id", "")))
rows.sort()
POLL = ("hipEventQuery", "hipStreamQuery")
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
polls = polls[-16:-1]
wait, tail, calls, period, names = [], [], [], [], {}
for k, (a, b, n, nxt) in enumerate(polls):
    wait.append((b - a) / 1e3)
    m = nxt
    seq = []
    while m < len(rows) and not rows[m][2].startswith("hipLaunchKernel") and not rows[m][2].startswith("hipModuleLaunch") and not rows[m][2].startswith("hipExtModuleLaunch"):
        seq.append(rows[m][2])
        m += 1
    if m < len(rows):
        tail.append((rows[m][0] - b) / 1e3)
        calls.append(len(seq))
        names[tuple(seq)] = names.get(tuple(seq), 0) + 1
    if k + 1 < len(polls):
        period.append((polls[k + 1][1] - b) / 1e3)
print("polls", len(polls), "queries per poll: mean %.0f" % st.mean(p[2] for p in polls))
print("poll, first query to its return: mean %.1f min %.1f max %.1f us" % (st.mean(wait), min(wait), max(wait)))
print("return of the poll to the start of the next kernel launch call: mean %.1f min %.1f max %.1f us, API calls in between: %s" % (st.mean(tail), min(tail), max(tail), sorted(set(calls))))
print("poll return to poll return (the host's step): mean %.1f min %.1f max %.1f us" % (st.mean(period), min(period), max(period)))
for seq, n in sorted(names.items(), key=lambda x: -x[1])[:3]:
    print(n, "x between poll and launch:", " ".join(seq))
