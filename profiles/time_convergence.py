"""Time of the per-dyad convergence pass (dlsm_convergence_accumulate: split R-hat and batch-means ESS of
every dyad) at the two sizes of time_ic.py, with S = 100 and S = 2000 samples (two chains' halves: 4 segments),
against dlsm_ic_accumulate on the same samples in the same process - the nearest existing pass: the same tiles,
the same staging of the samples, the same linear predictor, heavier transcendental work and four accumulators
per dyad instead of eight.  Both are timed with the chain's HIP events (Chain.timer_start / timer_stop on its
stream) after a warm-up call, host-to-device copies included on both sides; the median of REPEATS runs is
reported.  No threshold is set on the ratio.

    python profiles/time_convergence.py   # writes profiles/convergence_timing.json
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dynetlsm_amd as da                                  # noqa: E402

REPEATS = 5
SAMPLES = (100, 2000)
RHAT_EDGES = (1.01, 1.05, 1.1, 1.2, 1.5, 2.0)
ESS_EDGES = (10, 50, 100, 200, 400, 1000)


def measure(T, N, D, directed, S):
    # the pass does the same work whatever the samples hold: random positions, jittered
    rng = np.random.RandomState(1)
    Xs = np.empty((S, T, N, D))
    base = 1.5 * rng.randn(T, N, D)
    for s in range(S):                                      # (sample by sample: no second array of this size)
        Xs[s] = base + 0.05 * rng.randn(T, N, D)
    ic = np.stack([0.5 + 0.02 * rng.randn(S), (0.5 + 0.02 * rng.randn(S)) if directed else np.zeros(S)], axis=1)
    radii = rng.uniform(0.8, 1.25, (S, N)) if directed else None
    bits = np.zeros((T, N, da.engine.packed_row_words(N)), dtype=np.uint32)      # (an empty network)
    h = S // 4
    b = int(np.floor(np.sqrt(h)))
    out = dict(T=T, N=N, D=D, S=S, n_segments=4, seg_len=h, batch_len=b,
               model='directed' if directed else 'undirected')
    with da.Chain(T, N, D, 'directed' if directed else 'undirected') as c:

        def conv_call():
            return c.convergence_accumulate(Xs, ic, radii, n_segments=4, seg_len=h, batch_len=b,
                                            rhat_edges=RHAT_EDGES, ess_edges=ESS_EDGES)

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

        out['convergence_accumulate_ms'], out['convergence_accumulate_ms_runs'], res = timed(conv_call)
        out['ic_accumulate_ms'], out['ic_accumulate_ms_runs'], _ = timed(ic_call)
    n_dyads = int(res[0].sum())
    assert n_dyads == T * N * (N - 1) // (1 if directed else 2)
    out['ratio_convergence_over_ic'] = out['convergence_accumulate_ms'] / out['ic_accumulate_ms']
    out['dyad_samples_per_s'] = n_dyads * float(S) / (out['convergence_accumulate_ms'] * 1e-3)
    out['rhat_hist'] = [int(v) for v in res[0].sum(axis=0)]
    out['ess_hist'] = [int(v) for v in res[1].sum(axis=0)]
    return out


if __name__ == '__main__':
    cases = []
    for S in SAMPLES:
        for T, N, D, directed in ((10, 2000, 2, False), (5, 10000, 2, True)):
            cases.append(measure(T, N, D, directed, S))
            print(json.dumps(cases[-1]), flush=True)
    res = dict(what='dlsm_convergence_accumulate against dlsm_ic_accumulate on the same samples; HIP events, '
                    'median of %d' % REPEATS, cases=cases)
    path = os.path.join(ROOT, 'profiles', 'convergence_timing.json')
    json.dump(res, open(path, 'w'), indent=1)
    print(json.dumps(res))
