"""Developer tool: per-step figures from a rocprofv3 --kernel-trace csv of bench.py (one GPU, coverage pass on): durations of the clear, coverage_kernel and
render_kernel, the time between them, and where the pass of step k+1 lies relative to render_kernel of step k (profiles/coverage_overlap_ab.txt).
   rocprofv3 --kernel-trace --output-format csv -d <dir> -- python3 bench.py --gpus 1 --steps 100 --warmup 10
   python tools/coverage_trace_gaps.py <dir> 90          the last 90 steps"""
import csv
import glob
import statistics as st
import sys

d, n = sys.argv[1], int(sys.argv[2])
files = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
assert files, "no kernel trace under " + d
rows = []
for f in files:
    with open(f) as fh:
        for r in csv.DictReader(fh):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r.get("Queue_Id", "?"), r.get("Stream_Id", "?")))
rows.sort()
render = [r for r in rows if "render_kernel" in r[2]]
cover = [r for r in rows if "coverage_kernel" in r[2]]
fill = [r for r in rows if "fillBuffer" in r[2]]
print(f"{len(rows)} dispatches: render_kernel {len(render)}, coverage_kernel {len(cover)}, fillBuffer* {len(fill)}")
if len(render) != len(cover) or len(cover) <= n:
    sys.exit(f"this tool pairs every render_kernel with one coverage_kernel over the last {n} steps: the trace has frames without the coverage pass "
             "(mask off, a rank's tiles, a progressive frame), or fewer than n + 1 steps")
R, C = render[-n:], cover[-n:]
prev_c = cover[-n - 1][0]
F = []                                   # per step: the fills between the coverage kernel before and this one (the clear of the mask: one memset, one or two dispatches)
for c in C:
    F.append([f for f in fill if prev_c < f[0] < c[0]])
    prev_c = c[0]
if not all(F):
    sys.exit("a step has no fill dispatch in front of its coverage_kernel: not a trace of frames with the coverage pass")
us = lambda v: v / 1e3
med = lambda xs: f"median {us(st.median(xs)):8.2f} us  (min {us(min(xs)):8.2f}, max {us(max(xs)):8.2f})"
print(f"last {n} steps; queues: render {sorted(set(r[3] for r in R))} coverage {sorted(set(r[3] for r in C))}; streams: render {sorted(set(r[4] for r in R))} coverage {sorted(set(r[4] for r in C))}")
print("clear dispatches per step  ", sorted(set(len(f) for f in F)))
print("clear, summed durations    ", med([sum(x[1] - x[0] for x in f) for f in F]))
print("clear, first start->last end", med([f[-1][1] - f[0][0] for f in F]))
print("coverage_kernel duration   ", med([c[1] - c[0] for c in C]))
print("render_kernel duration     ", med([r[1] - r[0] for r in R]))
print("clear end -> coverage start", med([c[0] - f[-1][1] for f, c in zip(F, C)]))
print("coverage end -> render start (same step)", med([r[0] - c[1] for c, r in zip(C, R)]))
print("render end -> next step's clear start", med([F[k + 1][0][0] - R[k][1] for k in range(n - 1)]))
print("render end -> next render start", med([R[k + 1][0] - R[k][1] for k in range(n - 1)]))
print("render start -> next render start (step)", med([R[k + 1][0] - R[k][0] for k in range(n - 1)]))
inside = sum(1 for k in range(n - 1) if R[k][0] <= F[k + 1][0][0] and C[k + 1][1] <= R[k][1])
print(f"clear and coverage_kernel of step k+1 start and end inside render_kernel of step k: {inside} of {n - 1}")
inside_c = sum(1 for k in range(n - 1) if R[k][0] <= C[k + 1][0] and C[k + 1][1] <= R[k][1])
print(f"coverage_kernel of step k+1 starts and ends inside render_kernel of step k: {inside_c} of {n - 1}")
print("step k+1's clear start          - render_kernel k's start", med([F[k + 1][0][0] - R[k][0] for k in range(n - 1)]))
print("step k+1's coverage_kernel start - render_kernel k's start", med([C[k + 1][0] - R[k][0] for k in range(n - 1)]))
print("step k+1's coverage_kernel end   - render_kernel k's start", med([C[k + 1][1] - R[k][0] for k in range(n - 1)]))
print("step k+1's clear start          - render_kernel k-1's end ", med([F[k + 1][0][0] - R[k - 1][1] for k in range(1, n - 1)]))
