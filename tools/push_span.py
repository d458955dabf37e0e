#!/usr/bin/env python
"""Per owner-computes push call of a `rocprofv3 --kernel-trace` run of bench.py (rocpd .db): the sum of the kernel durations, the
span from the first kernel's start to the last kernel's end, and the per-kernel table -- span < sum means that kernels of the call
overlapped (the item chains of csrc/push_owner.hip).  argv: the .db [calls to average over, from the end = 20].

A call: from an own_zero (with the zero_fill right in front of it, the target's) up to the next own_zero or pull_sorted, in start
order; the push calls are the ones that hold own_accumulate launches."""
import re, sqlite3, sys


def short(name):
    m = re.search(r"(own_accumulate|own_bin|own_probe|own_zero|own_gather|zero_fill|push_tiled|pull_sorted)", name)    # (mangled names)
    return m.group(1) if m else name[:40]


def main():
    db = sqlite3.connect(sys.argv[1])
    last = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    rows = list(db.execute("""select s.kernel_name, d.start, d.end from rocpd_kernel_dispatch d
                              join rocpd_info_kernel_symbol s on d.kernel_id = s.id order by d.start"""))
    rows = [(short(n), a, b) for n, a, b in rows]
    calls, cur = [], None
    for i, (n, a, b) in enumerate(rows):
        if n == "own_zero" or n.startswith("pull_sorted"):
            if cur:
                calls.append(cur)
            cur = None
            if n == "own_zero":
                cur = [rows[i - 1]] if i and rows[i - 1][0] == "zero_fill" else []
                cur.append((n, a, b))
            continue
        if cur is not None:
            if n == "zero_fill" and i + 1 < len(rows) and rows[i + 1][0] == "own_zero":
                continue                                   # the next call's target
            cur.append((n, a, b))
    if cur:
        calls.append(cur)
    pushes = [c for c in calls if any(n == "own_accumulate" for n, _, _ in c)][-last:]
    if not pushes:
        print("no push calls found")
        return
    sums = [sum(b - a for _, a, b in c) / 1e3 for c in pushes]
    spans = [(max(b for _, _, b in c) - min(a for _, a, _ in c)) / 1e3 for c in pushes]
    print("push calls: %d   kernels per call: %d" % (len(pushes), len(pushes[0])))
    print("sum of kernel durations per call: mean %.1f us (min %.1f, max %.1f)" % (sum(sums) / len(sums), min(sums), max(sums)))
    print("span first start -> last end    : mean %.1f us (min %.1f, max %.1f)" % (sum(spans) / len(spans), min(spans), max(spans)))
    tab = {}
    for c in pushes:
        for n, a, b in c:
            t = tab.setdefault(n, [0, 0.0, 1e30, 0.0])
            d = (b - a) / 1e3
            t[0] += 1; t[1] += d; t[2] = min(t[2], d); t[3] = max(t[3], d)
    print("%-18s %9s %10s %10s %10s %12s" % ("kernel", "per call", "avg_us", "min_us", "max_us", "us per call"))
    for n, t in sorted(tab.items(), key=lambda kv: -kv[1][1]):
        print("%-18s %9.1f %10.1f %10.1f %10.1f %12.1f" % (n, t[0] / len(pushes), t[1] / t[0], t[2], t[3], t[1] / len(pushes)))


if __name__ == "__main__":
    main()
