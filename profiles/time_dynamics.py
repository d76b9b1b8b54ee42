"""Time of the tie dynamics pass (dlsm_dynamics_accumulate: per dyad and step Welford's moments of p_{t+1} - p_t,
three sums of probabilities and two counters in registers, the integer tables of the transitions; pointwise=False) at
the two sizes of time_ic.py, with S = 100 samples and min_count = 90, against dlsm_ic_accumulate and
dlsm_proba_accumulate on the same samples in the same process - the passes it shares its staging and its integer
tables with.  A step evaluates both of its time steps: (T - 1) steps cost 2 (T - 1) linear predictors per dyad and
sample where the other two cost T.  All three are timed with the chain's HIP events (Chain.timer_start / timer_stop
on its stream) after a warm-up call, host-to-device copies included on every side; the median of REPEATS runs is
reported.  No threshold is set on the ratios.

    python profiles/time_dynamics.py [--samples 100] [--shapes und,dir] [--out PATH]
                                                                # writes profiles/dynamics_timing.json

The cases of a run are merged into the file (a case of the same shape and S is replaced), so the cases can be run
one at a time.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dynetlsm_amd as da                                  # noqa: E402

REPEATS = 5
SAMPLES = (100,)
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
    min_count = int(np.ceil(LEVEL * S - 1e-12))
    out = dict(T=T, N=N, D=D, S=S, model='directed' if directed else 'undirected', level=LEVEL, min_count=min_count)
    with da.Chain(T, N, D, 'directed' if directed else 'undirected') as c:

        def dynamics_call():
            return c.dynamics_accumulate(bits, Xs, ic, radii, min_count)

        def proba_call():
            return c.proba_accumulate(bits, Xs, ic, radii, LEVEL)

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

        out['dynamics_accumulate_ms'], out['dynamics_accumulate_ms_runs'], res = timed(dynamics_call)
        out['ic_accumulate_ms'], out['ic_accumulate_ms_runs'], _ = timed(ic_call)
        out['proba_accumulate_ms'], out['proba_accumulate_ms_runs'], _ = timed(proba_call)
    n_steps = int(res[1].sum())
    assert n_steps == (T - 1) * N * (N - 1) // (1 if directed else 2) == int(res[0][..., 0].sum())
    out['ratio_dynamics_over_ic'] = out['dynamics_accumulate_ms'] / out['ic_accumulate_ms']
    out['ratio_dynamics_over_proba'] = out['dynamics_accumulate_ms'] / out['proba_accumulate_ms']
    # per linear predictor: a step forms two, the other passes one per time step
    out['ratio_per_eta_over_ic'] = out['ratio_dynamics_over_ic'] * T / (2.0 * (T - 1))
    out['step_samples_per_s'] = n_steps * float(S) / (out['dynamics_accumulate_ms'] * 1e-3)
    out['hist_up'] = [int(v) for v in res[1].sum(axis=0)]
    out['n_strengthened'] = int(res[2][..., 0].sum())
    out['n_weakened'] = int(res[2][..., 2].sum())
    return out


def merged(path, cases):
    """the file's content with ``cases`` in it: a case measured before at the same shape and S is replaced, the
    others stay, so that runs with --samples / --shapes add up to one file"""
    key = lambda c: (c['S'], c['N'], c['T'], c['D'], c['model'])
    kept = {}
    if os.path.exists(path):
        kept = {key(c): c for c in json.load(open(path))['cases']}
    kept.update({key(c): c for c in cases})
    return dict(what='dlsm_dynamics_accumulate (min_count = ceil(%g S), pointwise=False) against dlsm_ic_accumulate '
                     'and dlsm_proba_accumulate on the same samples; HIP events, median of %d; a case per run of the '
                     'script that measured it' % (LEVEL, REPEATS),
                cases=[kept[k] for k in sorted(kept)])


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', default=','.join(str(s) for s in SAMPLES))
    ap.add_argument('--shapes', default='und,dir')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dynamics_timing.json'))
    args = ap.parse_args()
    cases = []
    for S in [int(s) for s in args.samples.split(',')]:
        for shape in args.shapes.split(','):
            T, N, D, directed = SHAPES[shape]
            cases.append(measure(T, N, D, directed, S))
            print(json.dumps(cases[-1]), flush=True)
    json.dump(merged(args.out, cases), open(args.out, 'w'), indent=1)
    print(json.dumps(cases))
