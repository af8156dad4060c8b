"""Steady-state window of the headline in a rocprofv3 kernel trace of bench.py: summed kernel time against the wall time of
a step, and how long kernels of the two chains run at the same time.  usage: trace_stats.py t_kernel_trace.csv out.csv label"""
import csv
import sys

path, out, label = sys.argv[1:4]
rows = list(csv.DictReader(open(path)))
for r in rows:
    r["s"], r["e"] = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    r["wg"] = int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"])


def kind(r):
    n = r["Kernel_Name"]
    if "chain_step_kernel<6, 1, 6, 1" in n and "12>" in n:
        return "right"
    if "chain_step_kernel<3, 1, 3, 1" in n and "12>" in n:
        return "left"
    if "stream_small_kernel<6, 1" in n:
        return "psi"
    return "other"


right = sorted((r for r in rows if kind(r) == "right"), key=lambda r: r["s"])
assert len(right) >= 100, len(right)
t0, t1, steps = right[20]["s"], right[96]["s"], 19        # steps 5 .. 23 of the 25 (5 warm-up): from the first right step of one to that of the last
win = [r for r in rows if r["e"] > t0 and r["s"] < t1]
clip = lambda r: min(r["e"], t1) - max(r["s"], t0)


def union(rs):
    tot, cur_s, cur_e = 0, None, None
    for s, e in sorted((max(r["s"], t0), min(r["e"], t1)) for r in rs):
        if cur_e is None or s > cur_e:
            tot += (cur_e - cur_s) if cur_e is not None else 0
            cur_s, cur_e = s, e
        else:
            cur_e = max(cur_e, e)
    return tot + ((cur_e - cur_s) if cur_e is not None else 0)


def both(a, b):
    """time in the window during which a kernel of list a AND one of list b run"""
    return union(a) + union(b) - union(a + b)


by = {k: [r for r in win if kind(r) == k] for k in ("right", "left", "psi", "other")}
wall = (t1 - t0) / steps
res = [("label", label), ("steps_in_window", steps), ("wall_us_per_step", wall / 1e3),
       ("summed_kernel_us_per_step", sum(clip(r) for r in win) / steps / 1e3),
       ("busy_us_per_step", union(win) / steps / 1e3)]
for k, rs in by.items():
    res.append((k + "_launches_per_step", len(rs) / steps))
    res.append((k + "_avg_us", sum(r["e"] - r["s"] for r in rs) / max(1, len(rs)) / 1e3))
    res.append((k + "_workgroups", ",".join(sorted({str(r["wg"]) for r in rs})) if k != "other" else "-"))
res.append(("right_and_left_at_once_us_per_step", both(by["right"], by["left"]) / steps / 1e3))
res.append(("right_and_psi_at_once_us_per_step", both(by["right"], by["psi"]) / steps / 1e3))
res.append(("two_right_steps_at_once_us_per_step", (sum(clip(r) for r in by["right"]) - union(by["right"])) / steps / 1e3))
with open(out, "w") as f:
    w = csv.writer(f)
    w.writerow(["quantity", "value"])
    for k, v in res:
        w.writerow([k, ("%.1f" % v) if isinstance(v, float) else v])
        print(k, ("%.1f" % v) if isinstance(v, float) else v)
