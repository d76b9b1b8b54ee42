"""Time of the posterior edge probabilities pass (dlsm_proba_accumulate: Welford's moments of p and the two sorted
columns of every dyad in LDS, the integer tables of the calibration; pointwise=False) at the two sizes of
time_ic.py, with S = 100 (K = 6, four rows of dyads per workgroup) and S = 2000 samples (K = 101, one row), level
0.9, against dlsm_ic_accumulate and dlsm_loo_accumulate on the same samples in the same process - the pass it
shares its staging with, and the one it shares its tile forms and sorted insertion with.  All three are timed with
the chain's HIP events (Chain.timer_start / timer_stop on its stream) after a warm-up call, host-to-device copies
included on every side; the median of REPEATS runs is reported.  No threshold is set on the ratios.

    python profiles/time_proba.py [--samples 100,2000] [--shapes und,dir] [--out PATH]
                                                                # writes profiles/proba_timing.json

The cases of a run are merged into the file (a case of the same shape and S is replaced), so the long cases can be
run one at a time.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dynetlsm_amd as da                                  # noqa: E402
from dynetlsm_amd.loo import k_edges                       # noqa: E402

REPEATS = 5
SAMPLES = (100, 2000)
SHAPES = {'und': (10, 2000, 2, False), 'dir': (5, 10000, 2, True)}
LEVEL = 0.9


def measure(T, N, D, directed, S):
    # the passes do the same work whatever the samples hold: random positions, jittered, a sparse random network
    rng = np.random.RandomState(1)
    Xs = np.empty((S, T, N, D))
    base = 1.5 * rng.randn(T, N, D)
    for s in range(S):                                      # (sample by sample: no second array of this size)
        Xs[s] = base + 0.05 * rng.randn(T, N, D)
    ic = np.stack([0.5 + 0.02 * rng.randn(S), (0.5 + 0.02 * rng.randn(S)) if directed else np.zeros(S)], axis=1)
    radii = rng.uniform(0.8, 1.25, (S, N)) if directed else None
    bits = np.zeros((T, N, da.engine.packed_row_words(N)), dtype=np.uint32)      # (an empty network)
    edges = k_edges(S)
    out = dict(T=T, N=N, D=D, S=S, model='directed' if directed else 'undirected', level=LEVEL)
    with da.Chain(T, N, D, 'directed' if directed else 'undirected') as c:

        def proba_call():
            return c.proba_accumulate(bits, Xs, ic, radii, LEVEL)

        def loo_call():
            return c.loo_accumulate(bits, Xs, ic, radii, k_edges=edges)

        def ic_call():
            return c.ic_accumulate(bits, Xs, ic, radii)

        def timed(fn):
            fn()                                            # warm-up
            ms = []
            for _ in range(REPEATS):
                c.timer_start()
                r = fn()
                ms.append(c.timer_stop())
            return float(np.median(ms)), [float(m) for m in ms], r

        out['proba_accumulate_ms'], out['proba_accumulate_ms_runs'], res = timed(proba_call)
        out['ic_accumulate_ms'], out['ic_accumulate_ms_runs'], _ = timed(ic_call)
        out['loo_accumulate_ms'], out['loo_accumulate_ms_runs'], _ = timed(loo_call)
    n_dyads = int(res[3].sum())
    assert n_dyads == T * N * (N - 1) // (1 if directed else 2) == int(res[0][..., 0].sum())
    out['ratio_proba_over_ic'] = out['proba_accumulate_ms'] / out['ic_accumulate_ms']
    out['ratio_proba_over_loo'] = out['proba_accumulate_ms'] / out['loo_accumulate_ms']
    out['dyad_samples_per_s'] = n_dyads * float(S) / (out['proba_accumulate_ms'] * 1e-3)
    out['width_hist'] = [int(v) for v in res[3].sum(axis=0)]
    out['brier'] = float(sum(int(v) for v in res[1]) / 2.0 ** 32 / n_dyads)
    return out


def merged(path, cases):
    """the file's content with ``cases`` in it: a case measured before at the same shape and S is replaced, the
    others stay, so that runs with --samples / --shapes add up to one file"""
    key = lambda c: (c['S'], c['N'], c['T'], c['D'], c['model'])
    kept = {}
    if os.path.exists(path):
        kept = {key(c): c for c in json.load(open(path))['cases']}
    kept.update({key(c): c for c in cases})
    return dict(what='dlsm_proba_accumulate (level %g, pointwise=False) against dlsm_ic_accumulate and '
                     'dlsm_loo_accumulate on the same samples; HIP events, median of %d; a case per run of the '
                     'script that measured it' % (LEVEL, REPEATS),
                cases=[kept[k] for k in sorted(kept)])


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', default=','.join(str(s) for s in SAMPLES))
    ap.add_argument('--shapes', default='und,dir')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'proba_timing.json'))
    args = ap.parse_args()
    cases = []
    for S in [int(s) for s in args.samples.split(',')]:
        for shape in args.shapes.split(','):
            T, N, D, directed = SHAPES[shape]
            cases.append(measure(T, N, D, directed, S))
            print(json.dumps(cases[-1]), flush=True)
    json.dump(merged(args.out, cases), open(args.out, 'w'), indent=1)
    print(json.dumps(cases))
