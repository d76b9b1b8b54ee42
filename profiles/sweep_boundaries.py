"""Per-role durations of the LSM loop's launches from a rocprofv3 kernel trace (profiles/sweep_boundaries.md): the
sweep's launches with the head launch - the first k_pipe_step behind another kernel - apart from the others, the
resolve-only last launch, the likelihood pass and the fused last launch of the iteration.

    python profiles/sweep_boundaries.py <kernel_trace.csv> [launches to skip at the front]
"""
import csv
import sys
from collections import defaultdict

rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r['Start_Timestamp']))
rows = rows[int(sys.argv[2]) if len(sys.argv) > 2 else 0:]
groups = defaultdict(list)
prev = ''
for r in rows:
    name = r['Kernel_Name']
    short = name.split('(')[0].replace('void ', '').replace('dlsm::', '')
    d = int(r['End_Timestamp']) - int(r['Start_Timestamp'])
    if 'k_pipe_step' in name:
        groups[short + (' head' if 'k_pipe_step' not in prev else ' others')].append(d)
        groups[short + ' all'].append(d)
    else:
        groups[short].append(d)
    prev = name
lines = []
for g, v in sorted(groups.items(), key=lambda kv: -sum(kv[1])):
    s = sorted(v)
    lines.append('%-60s n=%6d  mean %8.3f us  median %8.3f us  total %10.1f us' %
                 (g, len(s), sum(s) / len(s) / 1e3, s[len(s) // 2] / 1e3, sum(s) / 1e3))
try:
    print('\n'.join(lines))
except BrokenPipeError:         # (piped into head)
    pass
