"""Time of the PSIS-LOO pass (dlsm_loo_accumulate: the sorted tail of every dyad in LDS, the generalised Pareto
fit and the smoothing after the last sample) at the two sizes of time_ic.py, with S = 100 (M = 20, four rows of
dyads per workgroup) and S = 2000 samples (M = 135, one row), against dlsm_ic_accumulate on the same samples in
the same process - the nearest existing pass: the same staging of the samples and the same pointwise
log-likelihood, four running moments per dyad instead of a sorted buffer.  Both are timed with the chain's HIP
events (Chain.timer_start / timer_stop on its stream) after a warm-up call, host-to-device copies included on
both sides; the median of REPEATS runs is reported.  No threshold is set on the ratio.

    python profiles/time_loo.py [--samples 100,2000] [--out PATH]   # writes profiles/loo_timing.json
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


def measure(T, N, D, directed, S):
    # the pass does the same work whatever the samples hold: random positions, jittered, a sparse random network
    rng = np.random.RandomState(1)
    Xs = np.empty((S, T, N, D))
    base = 1.5 * rng.randn(T, N, D)
    for s in range(S):                                      # (sample by sample: no second array of this size)
        Xs[s] = base + 0.05 * rng.randn(T, N, D)
    ic = np.stack([0.5 + 0.02 * rng.randn(S), (0.5 + 0.02 * rng.randn(S)) if directed else np.zeros(S)], axis=1)
    radii = rng.uniform(0.8, 1.25, (S, N)) if directed else None
    bits = np.zeros((T, N, da.engine.packed_row_words(N)), dtype=np.uint32)      # (an empty network)
    edges = k_edges(S)
    out = dict(T=T, N=N, D=D, S=S, model='directed' if directed else 'undirected', k_edges=[float(e) for e in edges])
    with da.Chain(T, N, D, 'directed' if directed else 'undirected') as c:

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

        out['loo_accumulate_ms'], out['loo_accumulate_ms_runs'], res = timed(loo_call)
        out['ic_accumulate_ms'], out['ic_accumulate_ms_runs'], _ = timed(ic_call)
    n_dyads = int(res[1].sum())
    assert n_dyads == T * N * (N - 1) // (1 if directed else 2)
    out['ratio_loo_over_ic'] = out['loo_accumulate_ms'] / out['ic_accumulate_ms']
    out['dyad_samples_per_s'] = n_dyads * float(S) / (out['loo_accumulate_ms'] * 1e-3)
    out['k_hist'] = [int(v) for v in res[1].sum(axis=0)]
    out['n_unfitted'] = int(res[0][:, 4].sum())
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', default=','.join(str(s) for s in SAMPLES))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'loo_timing.json'))
    args = ap.parse_args()
    cases = []
    for S in [int(s) for s in args.samples.split(',')]:
        for T, N, D, directed in ((10, 2000, 2, False), (5, 10000, 2, True)):
            cases.append(measure(T, N, D, directed, S))
            print(json.dumps(cases[-1]), flush=True)
    res = dict(what='dlsm_loo_accumulate against dlsm_ic_accumulate on the same samples; HIP events, '
                    'median of %d' % REPEATS, cases=cases)
    json.dump(res, open(args.out, 'w'), indent=1)
    print(json.dumps(res))
