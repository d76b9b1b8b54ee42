"""Time of the link prediction (top_dyads(model, k, n_samples=100): dlsm_topk_accumulate) at the two README shapes,
S = 100, k = 100 and k = 10 000, among='non_ties', against dlsm_score_accumulate - the same sample loop with the
log-loss terms next to it, the yardstick - and dlsm_ic_accumulate on the same samples in the same process.

The device calls are timed with the chain's HIP events (Chain.timer_start / timer_stop on its stream) after a
warm-up call, host-to-device copies and the host's step between the two launches included; the median of REPEATS
runs is reported.  The phases - k_topk_count with the histograms' memset, k_topk_threshold, k_topk_emit - come from
the event brackets of dlsm_profile_enable around each launch, in a run of their own.  The host's sort of the
candidates (engine.rank_candidates, part of the timed call) is timed once more by the host clock on the returned
dyads in shuffled order.  The fraction of tiles that the second launch revisits is what the call itself reports.

    python profiles/time_topk.py [--shapes und,dir] [--out PATH]        # writes profiles/topk_timing.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dynetlsm_amd as da                                  # noqa: E402
from dynetlsm_amd import _lib                              # noqa: E402

S, REPEATS = 100, 5
KS = (100, 10000)
SHAPES = {'und': (10, 2000, 2, False), 'dir': (5, 10000, 2, True)}


def measure(T, N, D, directed):
    # a random 3 % network, samples jittered around one configuration (profiles/time_scores.py)
    rng = np.random.RandomState(1)
    bits = np.zeros((T, N, da.engine.packed_row_words(N)), dtype=np.uint32)
    for t in range(T):
        A = rng.rand(N, N) < 0.03
        np.fill_diagonal(A, False)
        if not directed:
            A = np.triu(A, 1)
            A = A | A.T
        bits[t] = da.engine.pack_network(A[None])[0]
    Xs = np.empty((S, T, N, D))
    base = 1.5 * rng.randn(T, N, D)
    for s in range(S):                                      # (sample by sample: no second array of this size)
        Xs[s] = base + 0.05 * rng.randn(T, N, D)
    ic = np.stack([0.5 + 0.02 * rng.randn(S), (0.5 + 0.02 * rng.randn(S)) if directed else np.zeros(S)], axis=1)
    radii = rng.uniform(0.8, 1.25, (S, N)) if directed else None
    out = dict(T=T, N=N, D=D, S=S, model='directed' if directed else 'undirected', among='non_ties', k={})
    with da.Chain(T, N, D, 'directed' if directed else 'undirected') as c:

        def timed(fn):
            fn()                                            # warm-up
            ms = []
            for _ in range(REPEATS):
                c.timer_start()
                r = fn()
                ms.append(c.timer_stop())
            return float(np.median(ms)), [float(m) for m in ms], r

        out['score_accumulate_ms'], out['score_accumulate_ms_runs'], _ = timed(
            lambda: c.score_accumulate(bits, Xs, ic, radii))
        out['ic_accumulate_ms'], out['ic_accumulate_ms_runs'], _ = timed(lambda: c.ic_accumulate(bits, Xs, ic, radii))
        for k in KS:
            call = lambda: c.topk_accumulate(bits, Xs, ic, radii, k)             # noqa: E731
            row = {}
            row['topk_accumulate_ms'], row['topk_accumulate_ms_runs'], (steps, diag) = timed(call)
            row['ratio_topk_over_score'] = row['topk_accumulate_ms'] / out['score_accumulate_ms']
            row['ratio_topk_over_ic'] = row['topk_accumulate_ms'] / out['ic_accumulate_ms']
            c.profile_enable(True)
            for _ in range(REPEATS):
                call()
            row['phases_ms'] = {name: c.profile_read(slot)[0] / REPEATS
                                for name, slot in (('k_topk_count_and_memset_ms', _lib.K_TOPK_COUNT),
                                                   ('k_topk_threshold_ms', _lib.K_TOPK_SCAN),
                                                   ('k_topk_emit_ms', _lib.K_TOPK_EMIT))}
            c.profile_enable(False)
            # the host's sort of the candidates, on what came back
            raw = []
            for i, j, y, proba, sd in steps:
                perm = rng.permutation(i.size)
                raw.append((np.stack([i, j, y, 0 * y], axis=1).astype(np.int32)[perm],
                            np.stack([proba, sd], axis=1)[perm]))
            sort_ms = []
            for _ in range(REPEATS):
                t0 = time.perf_counter()
                again = [da.engine.rank_candidates(index, value, k) for index, value in raw]
                sort_ms.append((time.perf_counter() - t0) * 1e3)
            assert all(a[0].tobytes() == s[0].tobytes() and a[3].tobytes() == s[3].tobytes()
                       for a, s in zip(again, steps))
            row['host_sort_ms'] = float(np.median(sort_ms))
            row['tiles_revisited'] = int(diag['tiles_revisited'].sum())
            row['tiles'] = int(T * diag['n_tiles'])
            row['fraction_of_tiles_revisited'] = row['tiles_revisited'] / row['tiles']
            row['candidates_per_time_step'] = [int(v) for v in diag['n_beyond'] + diag['n_at']]
            row['eligible_per_time_step'] = [int(v) for v in diag['eligible']]
            row['smallest_returned_proba'] = float(min(s[3][-1] for s in steps))
            assert all(s[0].size == k for s in steps)
            out['k'][str(k)] = row
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='und,dir')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'topk_timing.json'))
    args = ap.parse_args()
    cases = []
    for shape in args.shapes.split(','):
        cases.append(measure(*SHAPES[shape]))
        print(json.dumps(cases[-1]), flush=True)
    res = dict(what='dlsm_topk_accumulate (among=non_ties, largest) against dlsm_score_accumulate and '
                    'dlsm_ic_accumulate on the same samples; HIP events, median of %d; phases by the event brackets '
                    'of dlsm_profile_enable' % REPEATS, cases=cases)
    json.dump(res, open(args.out, 'w'), indent=1)
