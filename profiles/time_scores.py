"""Time of the in-sample scores (in_sample_scores(model, n_samples=100): dlsm_score_accumulate) at the two
README shapes, against dlsm_ic_accumulate on the same inputs in the same process - the same per-dyad sample
loop without the histogram - and, at N = 2000, against the host path of ``auc_`` (probas_ + network_auc:
dense (T, N, N) float64 arrays and scikit-learn's sort).

The device calls are timed with the chain's HIP events (Chain.timer_start / timer_stop on its stream) after a
warm-up call, host-to-device copies included; the median of REPEATS runs is reported.  The parts of the call -
k_score_accumulate, the histograms' memset, k_score_scan with the pooling and the log-loss reduction - come
from the event brackets of dlsm_profile_enable around each launch, in a run of their own.  What the atomics
cost is not separable inside a launch: k_score_accumulate is also timed with one sample (its set-up, one pass
of the sample loop, the keys, the atomics and the log-loss terms) next to the run with all S.  The facade is
timed by the host clock around the whole call, the packing of the network on the host included.

    python profiles/time_scores.py            # writes profiles/scores_timing.json
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dynetlsm_amd as da                                  # noqa: E402
from dynetlsm_amd import _lib                              # noqa: E402
from dynetlsm_amd.metrics import FittedQuantities         # noqa: E402

S, REPEATS = 100, 5


class Fit(FittedQuantities):
    """the fitted attributes in_sample_scores and auc_ read, around a synthetic trace"""

    def __init__(self, Y, Xs, ic, radii, directed):
        self.is_directed = directed
        self.n_burn_ = 0
        self.Y_fit_ = Y
        self.Xs_, self.intercepts_, self.radiis_ = Xs, (ic if directed else ic[:, :1]), radii
        self.X_, self.intercept_ = Xs[-1], self.intercepts_[-1]
        self.radii_ = radii[-1] if directed else None


def measure(T, N, D, directed, host_path):
    # the pass does the same work whatever the network holds: a random 3 % network, samples jittered around
    # one configuration (profiles/time_ic.py)
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

        def timed(fn):
            fn()                                            # warm-up
            ms = []
            for _ in range(REPEATS):
                c.timer_start()
                r = fn()
                ms.append(c.timer_stop())
            return float(np.median(ms)), [float(m) for m in ms], r

        out['score_accumulate_ms'], out['score_accumulate_ms_runs'], (counts, ll) = timed(
            lambda: c.score_accumulate(bits, Xs, ic, radii))
        out['ic_accumulate_ms'], out['ic_accumulate_ms_runs'], (totals, _) = timed(
            lambda: c.ic_accumulate(bits, Xs, ic, radii))
        out['ratio_score_over_ic'] = out['score_accumulate_ms'] / out['ic_accumulate_ms']
        # the two passes agree on what they both compute: the log-loss sum is minus the sum of lppd
        out['max_rel_diff_logloss_vs_lppd'] = float(np.max(np.abs(ll + totals[:, 0]) / np.abs(ll)))
        # the parts, by the event brackets around each launch (a run of their own)
        parts = {}
        for label, n in (('S', S), ('one_sample', 1)):
            c.score_accumulate(bits, Xs[:n], ic[:n], None if radii is None else radii[:n])
            c.profile_enable(True)
            for _ in range(REPEATS):
                c.score_accumulate(bits, Xs[:n], ic[:n], None if radii is None else radii[:n])
            parts[label] = {name: c.profile_read(k)[0] / REPEATS
                            for name, k in (('k_score_accumulate_ms', _lib.K_SCORE_ACCUMULATE),
                                            ('memset_ms', _lib.K_SCORE_CLEAR),
                                            ('k_score_scan_ms', _lib.K_SCORE_SCAN))}
            c.profile_enable(False)
        out['parts_ms'] = parts['S']
        out['parts_ms_one_sample'] = parts['one_sample']
        kernels = sum(parts['S'].values())
        out['share_of_kernel_time'] = {
            'sample_loop': (parts['S']['k_score_accumulate_ms'] - parts['one_sample']['k_score_accumulate_ms'])
            / kernels,
            'set_up_keys_atomics_one_sample': parts['one_sample']['k_score_accumulate_ms'] / kernels,
            'memset': parts['S']['memset_ms'] / kernels, 'scan': parts['S']['k_score_scan_ms'] / kernels}
    res = da.scores.scores_from_counts(counts, ll, is_directed=directed)
    out['auc'], out['auc_bound'], out['log_loss'], out['n'] = res.auc, res.auc_bound, res.log_loss, res.n
    out['dyad_samples_per_s'] = res.n * S / (out['score_accumulate_ms'] * 1e-3)
    # the facade, by the host clock: packing the network and making the chain included
    model = Fit(Y, Xs, ic, radii, directed)
    da.in_sample_scores(model, n_samples=S)
    wall = []
    for _ in range(3):
        t0 = time.perf_counter()
        got = da.in_sample_scores(model, n_samples=S)
        wall.append((time.perf_counter() - t0) * 1e3)
    assert got.counts == res.counts
    out['in_sample_scores_wall_ms'], out['in_sample_scores_wall_ms_runs'] = float(np.median(wall)), wall
    if host_path:
        t0 = time.perf_counter()
        host_auc = model.auc_
        out['host_auc_wall_ms'] = (time.perf_counter() - t0) * 1e3
        point = da.in_sample_scores(model, estimate='map')
        out['host_auc'], out['device_map_auc'], out['device_map_auc_bound'] = host_auc, point.auc, point.auc_bound
    return out


if __name__ == '__main__':
    res = dict(what='dlsm_score_accumulate against dlsm_ic_accumulate on the same inputs; HIP events, median of %d; '
                    'parts by the event brackets of dlsm_profile_enable; facade and host path by the host clock'
                    % REPEATS,
               cases=[measure(10, 2000, 2, False, True), measure(5, 10000, 2, True, False)])
    path = os.path.join(ROOT, 'profiles', 'scores_timing.json')
    json.dump(res, open(path, 'w'), indent=1)
    print(json.dumps(res))
