#!/usr/bin/env python
"""Per-launch durations and launch-to-launch gaps of one forward, from a rocprofv3 kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o TAG -- python bench.py --batch 64 --no-extras --cpu-seconds 0
    python tools/kernel_trace_gaps.py DIR/**/TAG_kernel_trace.csv > profiles/TAG_kernel_trace.tsv
    python tools/kernel_trace_gaps.py BEFORE.csv AFTER.csv > profiles/TAG_before_after_kernel_trace.tsv

A forward starts at every dispatch whose kernel name contains --anchor (the stem kernel).  Forwards with the modal number of
launches are kept; per position the table gives the median over them of the kernel's duration and of the gap between its end
and the next launch's start (the last launch's gap runs into the next forward and is left out of the totals).  With two traces
the rows are joined by position and the difference of duration + gap is added: the cost of a launch as its successor sees it.
"""
import argparse
import csv
import re
import statistics
import sys


def short(name):
    name = re.sub(r'\(.*$', '', name)             # argument list of the demangled name
    name = re.sub(r'^void\s+', '', name)
    name = name.replace('metro::', '')
    return name if len(name) <= 70 else name[:67] + '...'


def forwards(path, anchor):
    with open(path, newline='') as f:
        rows = [r for r in csv.DictReader(f)]
    rows = [(int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name']) for r in rows]
    rows.sort()
    starts = [i for i, r in enumerate(rows) if anchor in r[2]]
    if len(starts) < 3:
        sys.exit(f'{path}: fewer than 3 launches of a kernel named *{anchor}*')
    seqs = [rows[a:b] for a, b in zip(starts, starts[1:])]           # the last forward has no successor: dropped
    nexts = [rows[b][0] for b in starts[1:]]
    n = statistics.mode(len(s) for s in seqs)
    keep = [(s, nx) for s, nx in zip(seqs, nexts) if len(s) == n]
    names = [r[2] for r in keep[0][0]]
    keep = [(s, nx) for s, nx in keep if [r[2] for r in s] == names]
    table = []
    for i, name in enumerate(names):
        dur = [s[i][1] - s[i][0] for s, _ in keep]
        gap = [(s[i + 1][0] if i + 1 < n else nx) - s[i][1] for s, nx in keep]
        table.append((short(name), statistics.median(dur) / 1e3, statistics.median(gap) / 1e3))
    return table, len(keep)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('trace', nargs='+', help='one kernel_trace.csv, or two: before after')
    ap.add_argument('--anchor', default='stem_pool', help='substring of the first kernel of a forward')
    a = ap.parse_args()
    if len(a.trace) > 2:
        ap.error('one or two traces')
    tabs = [forwards(p, a.anchor) for p in a.trace]
    t0, n0 = tabs[0]
    if len(tabs) == 1:
        print(f'# {a.trace[0]}: medians over {n0} forwards, microseconds')
        print('pos\tkernel\tdur_us\tgap_after_us')
        for i, (name, d, g) in enumerate(t0):
            print(f'{i}\t{name}\t{d:.2f}\t{g:.2f}')
        print(f'# sum of durations {sum(r[1] for r in t0):.1f} us, sum of gaps inside the forward {sum(r[2] for r in t0[:-1]):.1f} us')
        return
    t1, n1 = tabs[1]
    if [r[0] for r in t0] != [r[0] for r in t1]:
        sys.exit('the two traces do not run the same kernel sequence')
    print(f'# before {a.trace[0]} ({n0} forwards), after {a.trace[1]} ({n1} forwards): medians, microseconds')
    print('pos\tkernel\tdur_before\tgap_before\tdur_after\tgap_after\tdelta_dur_plus_gap')
    for i, ((name, d0, g0), (_, d1, g1)) in enumerate(zip(t0, t1)):
        print(f'{i}\t{name}\t{d0:.2f}\t{g0:.2f}\t{d1:.2f}\t{g1:.2f}\t{(d1 + g1) - (d0 + g0):+.2f}')
    for label, t in (('before', t0), ('after', t1)):
        print(f'# {label}: sum of durations {sum(r[1] for r in t):.1f} us, sum of gaps inside the forward '
              f'{sum(r[2] for r in t[:-1]):.1f} us')


if __name__ == '__main__':
    main()
