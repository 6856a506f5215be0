"""per kernel of the timed steps of a kernel trace: mean / min / max duration; and the gaps around k_route"""
import csv, glob, sys, statistics as st
rows = []
for f in glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0].split("::")[-1][:40]))
rows.sort()
# the steps: from a k_route to the next; the last 14 steps of the run (the timed loop is the end of the run, without legs)
idx = [i for i, r in enumerate(rows) if r[2] == "k_route"]       # (not k_route_tables / k_route_pos: once per upload)
steps = [(rows[a:b]) for a, b in zip(idx[:-1], idx[1:])][-15:-1]
dur, gap_next, start_after = {}, [], {}
for s, nxt in zip(steps, [x[0] for x in steps[1:]] + [None]):
    end_route = s[0][1]
    for (a, b, n) in s:
        dur.setdefault(n, []).append((b - a) / 1e3)
        start_after.setdefault(n, []).append((a - end_route) / 1e3)
    if nxt is not None:
        gap_next.append((nxt[0] - max(b for a, b, n in s)) / 1e3)
print("steps", len(steps), "kernels per step", sorted({len(s) for s in steps}))
for n, v in dur.items():
    print("%-42s n=%3d dur mean %7.1f min %7.1f max %7.1f us; start behind end of k_route %7.1f" % (n, len(v), st.mean(v), min(v), max(v), st.mean(start_after[n])))
if gap_next:
    print("gap from the step's last kernel end to the next k_route: mean %.1f min %.1f max %.1f us" % (st.mean(gap_next), min(gap_next), max(gap_next)))
