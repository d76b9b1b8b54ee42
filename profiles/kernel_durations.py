"""rocprofv3 --kernel-trace --stats summaries (profiles/rNN_kernel_stats_{lsm,hdp,cc}.csv) ->
profiles/kernel_durations.json: calls and average duration per kernel instantiation, the figure
`bench.py` divides the algorithmic flop by for `roofline.frac` (so that the fraction in the bench
line follows from the files under profiles/; the duration the run itself measures with events on
the launches is reported beside it).

    python profiles/kernel_durations.py r06 r07 > profiles/kernel_durations.json

(several tags: a later tag's files replace an earlier one's, model by model)
"""
import csv
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def short(name):
    """'void dlsm::k_pipe_step<2, 0, 1>(dlsm::ChainView, ...)' -> 'k_pipe_step<2,0,1>'"""
    n = name.split('(')[0].replace('void ', '').strip()
    n = n.split('::')[-1] if '<' not in n else re.sub(r'^.*?::(?=[A-Za-z_0-9]+<)', '', n)
    return n.replace(' ', '')


def main():
    # one tag, or several: a later tag's files replace an earlier one's, model by model
    tags = sys.argv[1:] or ['r04']
    out, used = {}, {}
    for tag in tags:
        for model in ('lsm', 'hdp', 'cc', 'ccu'):
            path = os.path.join(HERE, '%s_kernel_stats_%s.csv' % (tag, model))
            if not os.path.exists(path):
                continue
            rows = {}
            for r in csv.DictReader(open(path)):
                rows[short(r['Name'])] = {'calls': int(r['Calls']), 'avg_us': round(float(r['AverageNs']) / 1e3, 4),
                                          'pct': float(r['Percentage'])}
            out[model] = rows
            used[model] = tag
    by_tag = {}
    for model, tag in used.items():
        by_tag.setdefault(tag, []).append(model)
    files = ', '.join('profiles/%s_kernel_stats_{%s}.csv' % (tag, ','.join(sorted(by_tag[tag])))
                      for tag in sorted(by_tag, reverse=True))
    out['_source'] = ('%s (rocprofv3 --kernel-trace --stats of bench.py --model M --no-cpu --steps 50 --warmup 10 '
                      '--profile-steps 0)' % files)
    json.dump(out, sys.stdout, indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
