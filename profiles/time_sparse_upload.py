"""Cost of the edge-list upload (csrc/kernels_edges.hpp, Chain.upload_network_edges) next to what the dense calls
offer for the same network, in one run:

  * T=10, N=2000, undirected (config 1's shape, density 0.03): upload_network_edges against upload_network of the
    float64 tensor;
  * T=5, N=10 000, directed, about 20 ties per node (config 4's shape): upload_network_edges on a directed chain
    (packed rows) and on a case-control chain (degree and edge tables) against the host table build from the edge
    arrays, as synthetic_directed_from_model does it, plus upload_edges.  upload_network of the dense tensor is NOT
    run at this size: it would be 4 GB of float64.

Per call two figures, kept apart: ``device_ms``, the span between two HIP events on the chain's stream around the
call (Chain.timer_start / timer_stop: copies, memsets and kernels, and the host's gaps between them), and
``wall_ms``, the host clock around the call, which for the parent paths includes the host-side table build.  Each
path is warmed up WARMUP times, then the paths of a size alternate for REPEATS rounds; medians and minima.

    python profiles/time_sparse_upload.py [out.json]      # default: profiles/sparse_upload_timing.json
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dynetlsm_amd as da                                              # noqa: E402
from dynetlsm_amd.synthetic import synthetic_lsm_network, synthetic_directed_from_model     # noqa: E402

WARMUP, REPEATS = 3, 15


def host_tables(src, dst, T, N):
    """the parent's way from edge arrays to the padded tables (synthetic_directed_from_model's tail)"""
    degree = np.zeros((T, N, 2), dtype=np.int64)
    for t in range(T):
        degree[t, :, 1] = np.bincount(src[t], minlength=N)
        degree[t, :, 0] = np.bincount(dst[t], minlength=N)
    out_edges = np.zeros((T, N, max(1, int(degree[:, :, 1].max()))), dtype=np.int64)
    in_edges = np.zeros((T, N, max(1, int(degree[:, :, 0].max()))), dtype=np.int64)
    for t in range(T):
        # (the lists arrive sorted by source, targets increasing inside a row: no sort for the out table)
        start = np.concatenate([[0], np.cumsum(degree[t, :, 1])[:-1]])
        out_edges[t, src[t], np.arange(src[t].size) - start[src[t]]] = dst[t]
        order = np.lexsort((src[t], dst[t]))
        ds, ss = dst[t][order], src[t][order]
        start = np.concatenate([[0], np.cumsum(degree[t, :, 0])[:-1]])
        in_edges[t, ds, np.arange(ds.size) - start[ds]] = ss
    return in_edges, out_edges, degree


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


def main(path):
    out = dict(warmup=WARMUP, repeats=REPEATS)

    # ---- T=10, N=2000, undirected ------------------------------------------------------------------------
    T, N = 10, 2000
    net = synthetic_lsm_network(T=T, N=N, D=2, density=0.03, seed=0)
    Y = np.ascontiguousarray(net['Y'], dtype=np.float64)
    sp = da.SparseNetwork.from_dense(Y)
    with da.Chain(T, N, 2, 'undirected') as dense, da.Chain(T, N, 2, 'undirected') as edges:
        res = alternate({
            'upload_network_dense': (dense, lambda: dense.upload_network(Y)),
            'upload_network_edges': (edges, lambda: edges.upload_network_edges(sp)),
        })
        n = dense.network_packed_words()
        a, b = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        dense.get_network_packed(a.ctypes.data, n); edges.get_network_packed(b.ctypes.data, n)
        res['same_words'] = bool(np.array_equal(a, b))
    res.update(T=T, N=N, model='undirected', pairs_listed=int(sp.n_edges.sum()),
               dense_bytes=int(Y.nbytes), edge_list_bytes=int(8 * sp.n_edges.sum()))
    out['undirected_T10_N2000'] = res

    # ---- T=5, N=10 000, directed, ~20 ties per node --------------------------------------------------------
    T, N = 5, 10000
    net = synthetic_directed_from_model(T=T, N=N, mean_degree=20.0, seed=0)
    sp = net['network']
    offsets, src_all, dst_all = sp.by_time()
    src = [src_all[offsets[t]:offsets[t + 1]].astype(np.int64) for t in range(T)]
    dst = [dst_all[offsets[t]:offsets[t + 1]].astype(np.int64) for t in range(T)]

    def parent_tables(chain):
        ie, oe, dg = host_tables(src, dst, T, N)
        chain.upload_edges(ie, oe, dg)

    with da.Chain(T, N, 2, 'directed') as packed, da.Chain(T, N, 2, 'case_control') as cc, \
            da.Chain(T, N, 2, 'case_control') as parent:
        res = alternate({
            'packed_upload_network_edges': (packed, lambda: packed.upload_network_edges(sp)),
            'case_control_upload_network_edges': (cc, lambda: cc.upload_network_edges(sp)),
            'case_control_host_tables_upload_edges': (parent, lambda: parent_tables(parent)),
        })
        ie, oe, dg = cc.get_edge_tables()
        # (the host build pads an empty table to width 1; the widths agree whenever there is a tie)
        res['same_tables'] = bool(np.array_equal(dg, net['degree']) and np.array_equal(ie, net['in_edges']) and
                                  np.array_equal(oe, net['out_edges']))
        res['table_widths'] = list(cc.edge_table_widths())
    res.update(T=T, N=N, model='directed / case_control', pairs_listed=int(sp.n_edges.sum()),
               mean_out_degree=float(sp.n_edges.sum()) / (T * N), dense_bytes_not_run=int(8 * T * N * N),
               edge_list_bytes=int(8 * sp.n_edges.sum()),
               note='upload_network of the dense tensor was not run at this size (4 GB of float64)')
    out['directed_T5_N10000'] = res

    json.dump(out, open(path, 'w'), indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'sparse_upload_timing.json'))
