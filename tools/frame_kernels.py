"""Each kernel's place in the pipelined frame, from a rocprofv3 kernel trace (next to tools/frame_gaps.py, which gives
the frame's span, busy and idle time).

usage: python tools/frame_kernels.py <run_kernel_trace.csv> <first-kernel-of-frame substring> [skip frames]

Frames are cut at each launch of the named kernel (e.g. k_gbuffer).  Per kernel name, medians over the frames: its start
after the frame's first kernel started, its duration, the grid it ran (workgroups), and the idle gaps next to it: the
time just before its start, and just after its end, during which no kernel of any stream was running (0 when another
kernel was running at that moment)."""
import csv
import re
import statistics
import sys

rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r["Start_Timestamp"]))
mark, skip = sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 5
iv = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows]
starts = [i for i, r in enumerate(rows) if mark in r["Kernel_Name"]]


def short(name):
    m = re.search(r"\b(k_\w+)", name)
    return m.group(1) if m else name[:32]


def gap_before(i):
    s = iv[i][0]
    ends = [e for j, (b, e) in enumerate(iv[max(0, i - 16): i + 16], max(0, i - 16)) if j != i and b < s]
    if not ends or max(ends) >= s:
        return 0.0 if ends else float("nan")
    return (s - max(ends)) / 1e3


def gap_after(i):
    e = iv[i][1]
    near = [(b, x) for j, (b, x) in enumerate(iv[max(0, i - 16): i + 16], max(0, i - 16)) if j != i]
    if any(b <= e < x for b, x in near):
        return 0.0
    later = [b for b, x in near if b > e]
    return (min(later) - e) / 1e3 if later else float("nan")


stats = {}
for a, b in zip(starts[skip:], starts[skip + 1:]):
    t0 = iv[a][0]
    for i in range(a, b):
        r = rows[i]
        wg = (int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"])) * (int(r["Grid_Size_Y"]) // int(r["Workgroup_Size_Y"])) * \
             (int(r["Grid_Size_Z"]) // int(r["Workgroup_Size_Z"]))
        stats.setdefault(short(r["Kernel_Name"]), []).append(
            ((iv[i][0] - t0) / 1e3, (iv[i][1] - iv[i][0]) / 1e3, gap_before(i), gap_after(i), wg))
# the frame's time without any kernel, kernels of the frames before it that are still running included (frame_gaps.py
# counts a frame's own kernels only)
idle = []
for a, b in zip(starts[skip:], starts[skip + 1:]):
    t0, t1 = iv[a][0], iv[b][0]
    cur, u = t0, 0
    for s, e in sorted((max(s, t0), min(e, t1)) for s, e in iv[max(0, a - 16): b] if e > t0 and s < t1):
        if e > cur:
            u += e - max(s, cur)
            cur = e
    idle.append((t1 - t0 - u) / 1e3)
print(f"frames {len(starts) - skip - 1}: no kernel running for {statistics.median(idle):.1f} us of the median frame "
      f"(mean {statistics.fmean(idle):.1f} us)")
for name, v in stats.items():
    med = [statistics.median(x[k] for x in v) for k in range(5)]
    print(f"{name:24s} n {len(v):4d}  start {med[0]:7.1f} us  duration {med[1]:7.1f} us  idle before {med[2]:5.1f} us  "
          f"idle after {med[3]:5.1f} us  workgroups {int(med[4])}")
