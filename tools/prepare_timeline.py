"""The step's timeline from the compositing to the table scatter, from a rocprofv3 kernel trace
(``--kernel-trace --output-format csv``) of the bench command: for each of the LAST ``steps`` optimiser steps, when
every kernel between ``k_composite_wave`` and the end of the accumulation starts and ends, relative to the
compositing's end; the median over the steps per kernel (in launch order), and the scatter's start.  Shows
whether the backward's preparation (side branch) or the MLP backward (main branch) holds the scatter back.

    python tools/prepare_timeline.py run_kernel_trace.csv [steps] > profiles/<tag>_prepare_timeline_C2.json
"""
import csv
import json
import statistics
import sys

ANCHOR, SCATTER, LAST = "k_composite_wave", "k_bwd_scatter_rows", "k_bwd_accum"


def short(name):
    return name.split("(")[0].replace("void ", "").replace("lnr::", "").split("<")[0].strip()


def main(path, steps=20):
    steps = int(steps)
    ev = []
    for r in csv.DictReader(open(path)):
        ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"]),
                   int(r.get("Workgroup_Size_X") or r.get("Workgroup_Size") or 0), int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0)))
    ev.sort()
    anchors = [i for i, e in enumerate(ev) if e[2] == ANCHOR]
    rows = {}  # (kernel, occurrence in the step) -> [(start, end)] relative to the compositing's end, us
    order, shapes, used = [], {}, 0
    for a in range(max(len(anchors) - steps - 1, 0), len(anchors) - 1):
        i, nxt = anchors[a], anchors[a + 1]
        t0 = ev[i][1]
        seen, done = {}, False
        has_scatter = any(e[2] == SCATTER for e in ev[i + 1:nxt])
        if not has_scatter:
            continue  # (a step of the full backward, before the live switch)
        used += 1
        for s, e, name, wg, grid in ev[i + 1:nxt]:
            if done and not name.startswith(LAST):
                break
            occ = seen.get(name, 0)
            seen[name] = occ + 1
            key = f"{name}#{occ}" if occ else name
            if key not in rows:
                rows[key] = []
                order.append(key)
                shapes[key] = (grid // wg if wg else 0, wg)
            rows[key].append(((s - t0) / 1e3, (e - t0) / 1e3))
            done = done or name.startswith(LAST)
    med = statistics.median
    out = dict(trace=path.split("/")[-1], steps=used, zero="end of " + ANCHOR + " (us)", kernels=[])
    for key in order:
        v = rows[key]
        out["kernels"].append(dict(kernel=key, workgroups=shapes[key][0], threads=shapes[key][1], seen=len(v),
                                   start_us=round(med(a for a, _ in v), 1), end_us=round(med(b for _, b in v), 1),
                                   dur_us=round(med(b - a for a, b in v), 1)))
    sc = rows.get(SCATTER)
    if sc:
        out["scatter_start_us"] = dict(median=round(med(a for a, _ in sc), 1), min=round(min(a for a, _ in sc), 1),
                                       max=round(max(a for a, _ in sc), 1))
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main(*sys.argv[1:])
