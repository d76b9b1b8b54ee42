"""Cost of the missing-dyad imputation step (csrc/kernels_missing.hpp) at T=10, N=2000, d=2, undirected, 10 % of
the dyads missing: the step's launch against one full log-likelihood pass on the same chain in the same run,
and the device loop's iterations per second with the sampling on and off.

Each launch is bracketed by HIP events on the chain's stream (Chain.timer_start / timer_stop around one
enqueued step; the engine's own event brackets around the likelihood pass's kernel, Chain.profile_read), after
warm-up calls; medians / means of REPEATS launches.

    python profiles/missing_timing.py [out.json]      # default: profiles/missing_timing.json
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dynetlsm_amd as da                                  # noqa: E402
from dynetlsm_amd import _lib                               # noqa: E402
from dynetlsm_amd.model_selection import train_test_split  # noqa: E402
from dynetlsm_amd.synthetic import synthetic_lsm_network   # noqa: E402

T, N, D, SHARE, REPEATS, ITERS = 10, 2000, 2, 0.1, 50, 300


def main(path):
    net = synthetic_lsm_network(T=T, N=N, D=D, density=0.03, seed=0)
    _, index = train_test_split(net['Y'], SHARE, random_state=0)
    out = dict(T=T, N=N, D=D, model='undirected', missing_share=SHARE, n_missing=int(index.shape[0]),
               repeats=REPEATS)
    with da.Chain(T, N, D, 'undirected', seed=1) as c:
        c.upload_network(net['Y'])
        c.set_positions(net['X_init'])
        c.set_intercepts([net['intercept']])
        c.set_missing(index)
        for it in range(3):                                 # warm-up
            c.impute_missing(it)
            c.loglik_full()
        us = []
        for it in range(REPEATS):
            c.timer_start()
            c.impute_missing(10 + it)
            us.append(1e3 * c.timer_stop())
        out['impute_launch_us'] = float(np.median(us))
        out['impute_launch_us_min'] = float(np.min(us))
        # the likelihood pass: the engine's event bracket around its kernel, and the whole call
        c.profile_enable(True)
        for _ in range(REPEATS):
            c.loglik_full()
        ms, launches = c.profile_read(_lib.K_LOGLIK)
        c.profile_enable(False)
        out['loglik_pass_us'] = 1e3 * ms / launches
        us = []
        for _ in range(REPEATS):
            c.timer_start()
            c.loglik_full()
            us.append(1e3 * c.timer_stop())
        out['loglik_full_call_us'] = float(np.median(us))
        out['impute_over_loglik_pass'] = out['impute_launch_us'] / out['loglik_pass_us']
        out['condition_impute_no_longer_than_pass'] = bool(out['impute_launch_us'] <= out['loglik_pass_us'])
        # the device loop with and without the step
        c.set_prior_random_walk(2.0, 0.1)
        c.set_samplers(da.SamplerGrid(T, N, 0.1, tune=None))
        c.lsm_configure([net['intercept']], 2.0, tune=None)
        for key, on in (('iterations_per_s_sampling_off', False), ('iterations_per_s_sampling_on', True)):
            c.missing_sampling(on, accumulate_after=0)
            c.trace_alloc(ITERS + 21, logp0=0.0)
            c.lsm_run(1, 20)
            c.synchronize()
            t0 = time.perf_counter()
            c.lsm_run(21, ITERS)
            c.synchronize()
            out[key] = ITERS / (time.perf_counter() - t0)
        out['loop_cost_of_sampling'] = 1.0 - out['iterations_per_s_sampling_on'] / out['iterations_per_s_sampling_off']
    json.dump(out, open(path, 'w'), indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'missing_timing.json'))
