"""Cost of the missing lists' way onto the device (csrc/kernels_missing_edges.hpp, dlsm_set_missing_edges) next to
the host builder dlsm_set_missing on the same canonical list, in one run, and the host time of the sparse
``train_test_split`` that produces the list:

  * T=10, N=2000, undirected (density 0.03), 10 % of every slice's dyads held out;
  * T=5, N=10 000, directed, about 20 ties per node, 1 % of every slice's arcs held out.

Both entry points are called through the raw binding (no Python-side checks on either side), whole calls: the
host-to-device copies, the host builder's sort and the device builder's count read-back are inside.  Per call two
figures, kept apart: ``device_ms``, the span between two HIP events on the chain's stream around the call
(Chain.timer_start / timer_stop), and ``wall_ms``, the host clock around it.  Each path is warmed up WARMUP times,
then the paths of a size alternate for REPEATS rounds; medians and minima.

    python profiles/time_sparse_missing.py [out.json]      # default: profiles/sparse_missing_timing.json
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dynetlsm_amd as da                                              # noqa: E402
from dynetlsm_amd._lib import c_i32_p, c_i64_p                         # noqa: E402
from dynetlsm_amd.model_selection import train_test_split              # noqa: E402
from dynetlsm_amd.synthetic import synthetic_lsm_network, synthetic_directed_from_model     # noqa: E402

WARMUP, REPEATS = 3, 15


def alternate(paths):
    """{name: (chain, callable)} -> {name: {device_ms, wall_ms medians and minima}}, the paths taking turns"""
    for chain, call in paths.values():
        for _ in range(WARMUP):
            call()
        chain.synchronize()
    dev = {k: [] for k in paths}
    wall = {k: [] for k in paths}
    for _ in range(REPEATS):
        for name, (chain, call) in paths.items():
            chain.synchronize()
            t0 = time.perf_counter()
            chain.timer_start()
            call()
            dev[name].append(chain.timer_stop())
            wall[name].append(1e3 * (time.perf_counter() - t0))
    return {k: dict(device_ms=float(np.median(dev[k])), device_ms_min=float(np.min(dev[k])),
                    wall_ms=float(np.median(wall[k])), wall_ms_min=float(np.min(wall[k]))) for k in paths}


def one_shape(net, model, test_size):
    T, N, _ = net.shape
    directed = model == 'directed'
    t0 = time.perf_counter()
    net_train, index = train_test_split(net, test_size, random_state=0, is_directed=directed)
    split_s = time.perf_counter() - t0
    offsets, src, dst = net_train.missing_by_time()
    tij = np.ascontiguousarray(index, dtype=np.int32)

    def ok(chain, rc):
        if rc:
            raise RuntimeError(chain._L.dlsm_last_error(chain._h).decode())

    def edges(chain, allow_ties):
        ok(chain, chain._L.dlsm_set_missing_edges(chain._h, offsets.ctypes.data_as(c_i64_p),
                                                  src.ctypes.data_as(c_i32_p), dst.ctypes.data_as(c_i32_p),
                                                  allow_ties))

    def host(chain):
        ok(chain, chain._L.dlsm_set_missing(chain._h, tij.ctypes.data_as(c_i32_p), tij.shape[0]))

    with da.Chain(T, N, 2, model) as a, da.Chain(T, N, 2, model) as b, da.Chain(T, N, 2, model) as c:
        for chain in (a, b, c):
            chain.upload_network_edges(net_train)
        res = alternate({
            'set_missing_edges': (a, lambda: edges(a, 0)),
            'set_missing_edges_allow_ties': (b, lambda: edges(b, 1)),
            'set_missing_host_builder': (c, lambda: host(c)),
        })
        res['same_index'] = bool(np.array_equal(a.get_missing_index(), index) and
                                 np.array_equal(c.get_missing_index(), index))
    res.update(T=T, N=N, model=model, test_size=test_size, missing_dyads=int(index.shape[0]),
               ties_listed=int(net.n_edges.sum()), train_test_split_host_s=split_s)
    return res


def main(path):
    out = dict(warmup=WARMUP, repeats=REPEATS)
    Y = np.ascontiguousarray(synthetic_lsm_network(T=10, N=2000, D=2, density=0.03, seed=0)['Y'], dtype=np.float64)
    out['undirected_T10_N2000_10pct'] = one_shape(da.SparseNetwork.from_dense(Y), 'undirected', 0.1)
    net = synthetic_directed_from_model(T=5, N=10000, mean_degree=20.0, seed=0)['network']
    out['directed_T5_N10000_1pct'] = one_shape(net, 'directed', 0.01)
    json.dump(out, open(path, 'w'), indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'sparse_missing_timing.json'))
