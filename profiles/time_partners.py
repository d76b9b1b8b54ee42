"""Time of the per-node link prediction (top_partners(model, k, n_samples=100): dlsm_partners_accumulate) at the two
README shapes, S = 100, among='non_ties': every node with k = 10 and k = 64, and 100 random nodes (``rows=``, k = 10),
against dlsm_topk_accumulate (k = 100), the selection per time step on the same samples in the same process.

The device calls are timed with the chain's HIP events (Chain.timer_start / timer_stop on its stream) after a
warm-up call, host-to-device copies and the copy of the (T, N, k) lists back included; the median of REPEATS runs is
reported.  The kernel alone - k_partners_select - comes from the event bracket of dlsm_profile_enable around the
launch, in a run of its own.

    python profiles/time_partners.py [--shapes und,dir] [--out PATH]        # writes profiles/partners_timing.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dynetlsm_amd as da                                  # noqa: E402
from dynetlsm_amd import _lib                              # noqa: E402

S, REPEATS = 100, 5
K_TOPK = 100
SHAPES = {'und': (10, 2000, 2, False), 'dir': (5, 10000, 2, True)}


def measure(T, N, D, directed):
    # a random 3 % network, samples jittered around one configuration (profiles/time_topk.py)
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
    nodes = np.sort(rng.choice(N, 100, replace=False))
    out = dict(T=T, N=N, D=D, S=S, model='directed' if directed else 'undirected', among='non_ties', cases={})
    with da.Chain(T, N, D, 'directed' if directed else 'undirected') as c:

        def timed(fn):
            fn()                                            # warm-up
            ms = []
            for _ in range(REPEATS):
                c.timer_start()
                r = fn()
                ms.append(c.timer_stop())
            return float(np.median(ms)), [float(m) for m in ms], r

        out['topk_accumulate_ms'], out['topk_accumulate_ms_runs'], _ = timed(
            lambda: c.topk_accumulate(bits, Xs, ic, radii, K_TOPK))
        out['topk_k'] = K_TOPK
        for name, k, rows in (('k=10', 10, None), ('k=64', 64, None), ('k=10, 100 nodes', 10, nodes)):
            call = lambda: c.partners_accumulate(bits, Xs, ic, radii, k, rows=rows)      # noqa: E731
            row = dict(k=k, nodes=N if rows is None else int(rows.size))
            row['partners_accumulate_ms'], row['partners_accumulate_ms_runs'], got = timed(call)
            row['ratio_partners_over_topk'] = row['partners_accumulate_ms'] / out['topk_accumulate_ms']
            c.profile_enable(True)
            for _ in range(REPEATS):
                call()
            row['k_partners_select_ms'] = c.profile_read(_lib.K_PARTNERS)[0] / REPEATS
            c.profile_enable(False)
            partner, proba, sd, y, eligible = got
            asked = eligible[0] >= 0
            assert asked.sum() == row['nodes'] and (partner[:, asked] >= 0).all()
            row['row_blocks'] = int(np.unique(np.nonzero(asked)[0] // (32 if D <= 4 else 16)).size)
            row['smallest_returned_proba'] = float(np.nanmin(proba))
            row['median_kth_proba'] = float(np.median(proba[:, asked, k - 1]))
            out['cases'][name] = row
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='und,dir')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'partners_timing.json'))
    args = ap.parse_args()
    cases = []
    for shape in args.shapes.split(','):
        cases.append(measure(*SHAPES[shape]))
        print(json.dumps(cases[-1]), flush=True)
    res = dict(what='dlsm_partners_accumulate (among=non_ties, largest) against dlsm_topk_accumulate (k=%d) on the '
                    'same samples; HIP events, median of %d; the kernel by the event bracket of dlsm_profile_enable'
                    % (K_TOPK, REPEATS), cases=cases)
    json.dump(res, open(args.out, 'w'), indent=1)
