"""Time of the goodness-of-fit families over time against the structural family, which is the code path
of the check before they existed: for S posterior samples the device calls posterior_predictive_check
makes - 'structural': dlsm_gof_simulate; 'temporal' / 'geodesic': dlsm_gof_dynamic_simulate with that
family alone; 'all': both calls, every family - at T=10 N=2000 undirected (S = 100) and T=5 N=10 000
directed (S = 10), networks of about 3 % density.  Each is timed with the chain's HIP events
(Chain.timer_start / timer_stop on its stream) after a warm-up call, copies included; the median of
REPEATS runs is reported with the ratio to 'structural'.

    python profiles/time_gof_dynamic.py            # writes profiles/gof_dynamic_timing.json
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dynetlsm_amd as da                                  # noqa: E402

REPEATS = 3


def _density(X, b, directed, radii):
    d = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1))
    eta = b * (2 - d / radii[None, :] - d / radii[:, None]) if directed else b - d
    p = 1.0 / (1.0 + np.exp(-eta))
    return (p.sum() - np.trace(p)) / (len(X) * (len(X) - 1))


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
        calls = {
            'structural': lambda: c.gof_simulate(Xs, ic, radii, seed=7),
            'temporal': lambda: c.gof_dynamic_simulate(Xs, ic, radii, seed=7, geodesic=False),
            'geodesic': lambda: c.gof_dynamic_simulate(Xs, ic, radii, seed=7, temporal=False),
            'all': lambda: (c.gof_simulate(Xs, ic, radii, seed=7), c.gof_dynamic_simulate(Xs, ic, radii, seed=7)),
        }
        results = {}
        for name, fn in calls.items():
            results[name] = fn()                            # warm-up
            ms = []
            for _ in range(REPEATS):
                c.timer_start()
                fn()
                ms.append(c.timer_stop())
            out[name + '_ms'] = float(np.median(ms))
            out[name + '_ms_runs'] = [float(m) for m in ms]
            print('%s N=%d %s: %.1f ms' % (out['model'], N, name, out[name + '_ms']), flush=True)
    stats = results['structural']
    geo = results['geodesic'][2]
    out['density'] = float(stats[..., 0].mean() / (N * (N - 1) / (1.0 if directed else 2.0)))
    out['unreachable_share'] = float(geo[..., 0].sum() / geo.sum())
    out['longest_geodesic'] = int(np.nonzero(geo.reshape(-1, N).sum(0))[0].max())
    assert (geo[..., 1] == stats[..., 0]).all()             # the families describe the same draws
    for name in ('temporal', 'geodesic', 'all'):
        out['ratio_%s_over_structural' % name] = out[name + '_ms'] / out['structural_ms']
    return out


if __name__ == '__main__':
    res = dict(what='device calls of posterior_predictive_check per statistics family; HIP events, copies '
                    'included, median of %d' % REPEATS,
               cases=[measure(10, 2000, 2, False, 100), measure(5, 10000, 2, True, 10)])
    path = os.path.join(ROOT, 'profiles', 'gof_dynamic_timing.json')
    json.dump(res, open(path, 'w'), indent=1)
    print(json.dumps(res))
