"""Time of the multi-step posterior predictive forecast (forecast(model, horizon=H): dlsm_forecast_paths) at the two
README shapes - T=10 N=2000 K=20 undirected (the mixture dynamics of the HDP-LPCM) and T=5 N=10 000 directed (the
random walk of the LSM) - with S = 100 trajectories and H = 1 and 5, and next to the undirected case the only
comparable path the engine had before: ``forecast_probas_pp_`` (H = 1, undirected HDP-LPCM; labels and positions
drawn on the host in a Python loop over the samples, then uploaded for the mean), timed in the same run.

The device call is timed with the chain's HIP events (Chain.timer_start / timer_stop on its stream) after a
warm-up call, host-to-device and device-to-host copies included (the (H, N, N) result is most of the bytes at
N = 10 000); the median of REPEATS runs is reported.  The facade and ``forecast_probas_pp`` are timed by the host
clock around the whole call.  No speed-up is promised: the two paths draw from different generators, and the old
one renormalises the weights to the active components.

    python profiles/time_forecast.py            # writes profiles/forecast_timing.json
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dynetlsm_amd as da                                  # noqa: E402
from dynetlsm_amd import forecast as one_step              # noqa: E402

S, REPEATS = 100, 5


class Fit(object):
    """the fitted attributes forecast() and forecast_probas_pp read, around a synthetic trace"""
    n_burn_, thin, random_state, sigma_sq, n_features = 0, None, 0, 0.05, 2

    def __init__(self, rng, T, N, D, K, directed):
        self.is_directed = directed
        self.Y_fit_ = np.zeros((1, 1, 1))
        self.Xs_ = 1.5 * rng.randn(1, T, N, D) + 0.05 * rng.randn(S, T, N, D)
        self.intercepts_ = 0.5 + 0.02 * rng.randn(S, 2 if directed else 1)
        self.radiis_ = rng.uniform(0.8, 1.25, (S, N)) if directed else None
        self.X_, self.intercept_ = self.Xs_[-1], self.intercepts_[-1]
        self.radii_ = self.radiis_[-1] if directed else None
        if K:
            self.zs_ = rng.randint(0, K, (S, T, N))
            self.weights_ = rng.gamma(1.0, 1.0, (S, T, K, K)) + 1e-3
            self.betas_ = np.full((S, K), 1.0 / K)
            self.mus_ = 1.5 * rng.randn(S, K, D)
            self.sigmas_ = rng.uniform(0.05, 0.3, (S, K))
            self.lambdas_ = rng.uniform(0.7, 0.9, (S, 1))


def measure(T, N, D, K, directed, old_path):
    rng = np.random.RandomState(1)
    model = Fit(rng, T, N, D, K, directed)
    out = dict(T=T, N=N, D=D, K=K, S=S, model='directed' if directed else 'undirected',
               dynamics='mixture' if K else 'random walk')
    with da.Chain(1, N, D, 'directed' if directed else 'undirected') as c:
        model.chain_ = c
        for H in (1, 5):
            da.forecast(model, horizon=H)                    # warm-up
            ms, wall = [], []
            for _ in range(REPEATS):
                t0 = time.perf_counter()
                c.timer_start()
                res = da.forecast(model, horizon=H)
                ms.append(c.timer_stop())
                wall.append((time.perf_counter() - t0) * 1e3)
            out['forecast_H%d_ms' % H], out['forecast_H%d_ms_runs' % H] = float(np.median(ms)), [float(m) for m in ms]
            out['forecast_H%d_wall_ms' % H] = float(np.median(wall))
            out['mean_proba_H%d' % H] = float(res.probas[-1].sum() / (N * (N - 1)))
            del res
        if old_path:
            one_step.forecast_probas_pp(model, c)            # warm-up
            wall = []
            for _ in range(3):
                t0 = time.perf_counter()
                P = one_step.forecast_probas_pp(model, c)
                wall.append((time.perf_counter() - t0) * 1e3)
            out['forecast_probas_pp_wall_ms'], out['forecast_probas_pp_wall_ms_runs'] = float(np.median(wall)), wall
            out['forecast_probas_pp_mean_proba'] = float(P.sum() / (N * (N - 1)))
        del model.chain_
    return out


if __name__ == '__main__':
    res = dict(what='forecast(model, horizon=H) with S = %d trajectories: HIP events around the call (copies included) '
                    'and the host clock, median of %d; forecast_probas_pp (H = 1, undirected HDP-LPCM, host draws) '
                    'by the host clock in the same run' % (S, REPEATS),
               cases=[measure(10, 2000, 2, 20, False, True), measure(5, 10000, 2, 0, True, False)])
    path = os.path.join(ROOT, 'profiles', 'forecast_timing.json')
    json.dump(res, open(path, 'w'), indent=1)
    print(json.dumps(res))
