"""Time of the triadic goodness-of-fit family against the structural family on the same posterior samples:
the device calls posterior_predictive_check makes - 'structural': dlsm_gof_simulate; 'triadic':
dlsm_gof_triads_simulate - at T=10 N=2000 undirected (S = 100) and T=5 N=10 000 directed (S = 10), networks
of about 3 % density (the shapes and samples of profiles/time_gof_dynamic.py).  Both draw the same networks,
so the difference is the statistics kernel: k_gof_stats against k_gof_triads.  After a warm-up call of each,
the two are timed in turn, REPEATS times, with the chain's HIP events (Chain.timer_start / timer_stop on its
stream), copies included; the median is reported with the ratio to 'structural'.

    python profiles/time_gof_triads.py [out.json]     # default: profiles/gof_triads_timing.json
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dynetlsm_amd as da                                  # noqa: E402
from time_gof_dynamic import _density                      # noqa: E402

REPEATS = 5


def measure(T, N, D, directed, S, density=0.03):
    rng = np.random.RandomState(1)
    base = rng.randn(1, T, N, D) + 0.03 * rng.randn(S, T, N, D)
    radii = rng.uniform(0.8, 1.25, (S, N)) if directed else None
    b = 3.0 if directed else 0.5
    # the spread of the positions that gives the wanted density, by bisection on 500 nodes of the first sample
    sub = slice(0, min(N, 500))
    lo, hi = 0.1, 100.0
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        dens = _density(mid * base[0, 0, sub], b, directed, radii[0, sub] if directed else None)
        lo, hi = (lo, mid) if dens < density else (mid, hi)
    Xs = 0.5 * (lo + hi) * base
    ic = np.full((S, 2), b)
    if not directed:
        ic[:, 1] = 0.0
    out = dict(T=T, N=N, D=D, S=S, model='directed' if directed else 'undirected')
    with da.Chain(T, N, D, 'directed' if directed else 'undirected') as c:
        calls = {'structural': lambda: c.gof_simulate(Xs, ic, radii, seed=7),
                 'triadic': lambda: c.gof_triads_simulate(Xs, ic, radii, seed=7)}
        results = {name: fn() for name, fn in calls.items()}            # warm-up
        ms = {name: [] for name in calls}
        for _ in range(REPEATS):
            for name, fn in calls.items():
                c.timer_start()
                fn()
                ms[name].append(c.timer_stop())
    for name in calls:
        out[name + '_ms'] = float(np.median(ms[name]))
        out[name + '_ms_runs'] = [float(m) for m in ms[name]]
        print('%s N=%d %s: %.1f ms' % (out['model'], N, name, out[name + '_ms']), flush=True)
    stats = da.gof.derive_statistics(results['structural'], N, directed)
    tri = da.gof.derive_triad_statistics(results['triadic'], N, directed)
    out['density'] = float(stats['edges'].mean() / (N * (N - 1) / (1.0 if directed else 2.0)))
    # the families describe the same draws
    if directed:
        assert (tri['dyad_census'][..., 0] == stats['mutual']).all()
        assert (tri['dyad_census'][..., 1] + 2 * tri['dyad_census'][..., 0] == stats['edges']).all()
    else:
        assert (tri['triad_census'][..., 3] == stats['triangles']).all()
    out['connected_pairs_per_network'] = float(tri['dyad_census'][..., :2].sum(-1).mean())
    out['triad_transitivity'] = float(tri['triad_transitivity'].mean())
    out['ratio_triadic_over_structural'] = out['triadic_ms'] / out['structural_ms']
    return out


if __name__ == '__main__':
    res = dict(what='device calls of posterior_predictive_check, triadic against structural family on the same '
                    'samples, timed in turn; HIP events, copies included, median of %d' % REPEATS,
               cases=[measure(10, 2000, 2, False, 100), measure(5, 10000, 2, True, 10)])
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'gof_triads_timing.json')
    json.dump(res, open(path, 'w'), indent=1)
    print(json.dumps(res))
