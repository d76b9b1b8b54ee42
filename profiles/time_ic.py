"""Time of the information-criteria pass (dlsm_ic_accumulate, S = 100 samples) against the only other route
to any of its numbers: a host loop of S x (set the sample's state, dlsm_loglik_full) on the same chain,
which yields sample_loglik alone.  Both are timed with the chain's HIP events (Chain.timer_start /
timer_stop on its stream) after a warm-up call, host-to-device copies included on both sides; the median
of REPEATS runs is reported.

    python profiles/time_ic.py            # writes profiles/ic_timing.json
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dynetlsm_amd as da                                  # noqa: E402

S, REPEATS = 100, 5


def measure(T, N, D, directed):
    # the pass does the same work whatever the network holds: random positions, a random 3 % network
    rng = np.random.RandomState(1)
    Y = np.zeros((T, N, N))
    for t in range(T):
        A = (rng.rand(N, N) < 0.03).astype(np.float64)
        np.fill_diagonal(A, 0.0)
        if not directed:
            A = np.triu(A, 1)
            A = A + A.T
        Y[t] = A
    Xs = 1.5 * rng.randn(1, T, N, D) + 0.05 * rng.randn(S, T, N, D)
    ic = np.stack([0.5 + 0.02 * rng.randn(S), (0.5 + 0.02 * rng.randn(S)) if directed else np.zeros(S)], axis=1)
    radii = rng.uniform(0.8, 1.25, (S, N)) if directed else None
    bits = da.engine.pack_network(Y)
    out = dict(T=T, N=N, D=D, S=S, model='directed' if directed else 'undirected')
    with da.Chain(T, N, D, 'directed' if directed else 'undirected') as c:
        c.upload_network(Y)

        def ic_call():
            return c.ic_accumulate(bits, Xs, ic, radii)

        def loop():
            ll = np.zeros(S)
            for s in range(S):
                c.set_positions(Xs[s])
                c.set_intercepts(ic[s] if directed else ic[s, :1])
                if directed:
                    c.set_radii(radii[s])
                ll[s] = c.loglik_full()
            return ll

        def timed(fn):
            fn()                                            # warm-up
            ms = []
            for _ in range(REPEATS):
                c.timer_start()
                r = fn()
                ms.append(c.timer_stop())
            return float(np.median(ms)), [float(m) for m in ms], r

        out['ic_accumulate_ms'], out['ic_accumulate_ms_runs'], (totals, sl) = timed(ic_call)
        out['loglik_loop_ms'], out['loglik_loop_ms_runs'], ll = timed(loop)
    out['ratio_loop_over_ic'] = out['loglik_loop_ms'] / out['ic_accumulate_ms']
    out['max_rel_diff_sample_loglik'] = float(np.max(np.abs(sl.sum(axis=1) - ll) / np.abs(ll)))
    out['dyad_samples_per_s'] = float(totals[:, 4].sum()) * S / (out['ic_accumulate_ms'] * 1e-3)
    return out


if __name__ == '__main__':
    res = dict(what='dlsm_ic_accumulate against S x (set state, dlsm_loglik_full); HIP events, median of %d' % REPEATS,
               cases=[measure(10, 2000, 2, False), measure(5, 10000, 2, True)])
    path = os.path.join(ROOT, 'profiles', 'ic_timing.json')
    json.dump(res, open(path, 'w'), indent=1)
    print(json.dumps(res))
