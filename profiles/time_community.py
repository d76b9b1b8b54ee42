"""Time of the community pass (dlsm_community_accumulate: per labelling the cluster table, per node its ties into its
own cluster and its label changes; no blocks) at T=10 N=2000 K=20 undirected (density 0.03) and T=5 N=10 000 K=20
directed (20 out-ties a node), for S = 100 and S = 2000 labellings, against what it is compared with:

  - dlsm_post_cooccurrence on the same labels in the same process - the other pass over the stored labels;
  - the dense host formula of the reference, trace(S^T B S) / (2m) per time step (tests/community_ref.py), for
    S = 100 labellings at the first shape - what a user has without this pass, for the modularity alone.

The device calls are timed with the chain's HIP events (Chain.timer_start / timer_stop on its stream) after a warm-up
call; the label checks on the host and the copies in both directions are inside on every side; the median of REPEATS
runs is reported; ``community_kernels_ms`` is the three kernels' share of one call, from the chain's event brackets
(dlsm_profile_enable).  The networks are planted partitions of 20 groups, the labellings the planted one with 5 % of the
nodes relabelled at random per sample.  No threshold is set on any ratio.

    python profiles/time_community.py [--samples 100,2000] [--shapes und,dir] [--out PATH]
                                                                # writes profiles/community_timing.json

The cases of a run are merged into the file (a case of the same shape and S is replaced), so the cases can be run
one at a time.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import dynetlsm_amd as da                                  # noqa: E402
import community_ref                                       # noqa: E402

REPEATS = 5
SAMPLES = (100, 2000)
K = 20
SHAPES = {'und': (10, 2000, False), 'dir': (5, 10000, True)}
HOST_SAMPLES = 100                                         # labellings of the dense host formula ('und' only)


def planted_network(T, N, directed, rng):
    """(packed bits (T, N, W), planted labels (T, N)): ties mostly inside the groups.  Undirected: density 0.03, dense
    draws; directed: 20 out-neighbours a node, 16 of them from its own group, drawn as lists - no (N, N) array"""
    W = da.engine.packed_row_words(N)
    z = np.empty((T, N), dtype=np.int64)
    z[0] = rng.randint(0, K, size=N)
    for t in range(1, T):
        z[t] = np.where(rng.rand(N) < 0.05, rng.randint(0, K, size=N), z[t - 1])
    if not directed:
        Y = np.zeros((T, N, N), dtype=bool)
        for t in range(T):
            p = np.where(z[t][:, None] == z[t][None, :], 0.03 * 0.8 * K, 0.03 * 0.2 * K / (K - 1))
            A = np.triu(rng.rand(N, N) < p, 1)
            Y[t] = A | A.T
        return da.engine.pack_network(Y), z
    bits = np.zeros((T, N, W), dtype=np.uint32)
    for t in range(T):
        order = np.argsort(z[t], kind='stable')
        start = np.searchsorted(z[t][order], np.arange(K + 1))
        size = np.maximum(start[1:] - start[:-1], 1)
        own = order[np.minimum(start[z[t]][:, None] + (rng.rand(N, 16) * size[z[t]][:, None]).astype(np.int64), N - 1)]
        j = np.concatenate([own, rng.randint(0, N, size=(N, 4))], axis=1)
        i = np.repeat(np.arange(N), j.shape[1])
        j = j.ravel()
        keep = i != j
        np.bitwise_or.at(bits[t], (i[keep], j[keep] >> 5), np.uint32(1) << (j[keep] & 31).astype(np.uint32))
    return bits, z


def measure(T, N, directed, S, host_samples):
    rng = np.random.RandomState(1)
    bits, z = planted_network(T, N, directed, rng)
    zs = np.broadcast_to(z, (S, T, N)).copy()
    noise = rng.rand(S, T, N) < 0.05
    zs[noise] = rng.randint(0, K, size=int(noise.sum()))
    out = dict(T=T, N=N, K=K, S=S, model='directed' if directed else 'undirected',
               ties_per_step=int(np.unpackbits(bits[0].view(np.uint8)).sum()))       # ordered, at t = 0
    with da.Chain(T, N, 2, 'directed' if directed else 'undirected') as c:

        def timed(fn):
            fn()                                            # warm-up
            ms, wall = [], []
            for _ in range(REPEATS):
                t0 = time.perf_counter()
                c.timer_start()
                r = fn()
                ms.append(c.timer_stop())
                wall.append(1e3 * (time.perf_counter() - t0))
            return float(np.median(ms)), [float(m) for m in ms], float(np.median(wall)), r

        (out['community_accumulate_ms'], out['community_accumulate_ms_runs'], out['community_accumulate_wall_ms'],
         res) = timed(lambda: c.community_accumulate(bits, zs, K))
        print('community %s S=%d: %.2f ms' % (out['model'], S, out['community_accumulate_ms']), flush=True)
        (out['post_cooccurrence_ms'], out['post_cooccurrence_ms_runs'], out['post_cooccurrence_wall_ms'],
         _) = timed(lambda: c.post_cooccurrence(zs, K, want_matrix=False))
        c.post_release()
        # the three kernels' share of a call (label packing, the walk, the label changes): the chain's event brackets
        c.profile_enable(True)
        before = c.profile_read(da._lib.K_LABELS)[0]
        c.community_accumulate(bits, zs, K)
        out['community_kernels_ms'] = c.profile_read(da._lib.K_LABELS)[0] - before
        c.profile_enable(False)
    clusters = res[0]
    assert (clusters[..., 0].sum(-1) == N).all() and (clusters[..., 2].sum(-1) == out['ties_per_step'])[:, 0].all()
    q = da.community.modularity_from_clusters(clusters, directed)
    out['modularity_mean'] = float(np.nanmean(q))
    out['nodes_moved_per_step'] = float(res[3].mean())
    out['ratio_community_over_cooccurrence'] = out['community_accumulate_ms'] / out['post_cooccurrence_ms']
    out['labellings_per_s'] = S * T / (out['community_accumulate_ms'] * 1e-3)
    if host_samples and not directed and S >= host_samples:
        Y = np.unpackbits(bits.view(np.uint8), axis=-1, bitorder='little')[:, :, :N]
        t0 = time.perf_counter()
        dense = np.array([community_ref.dense_modularity(Y, zs[s], directed)[0] for s in range(host_samples)])
        out['host_dense_modularity_ms'] = 1e3 * (time.perf_counter() - t0)
        out['host_dense_modularity_samples'] = host_samples
        out['host_dense_max_abs_diff'] = float(np.abs(dense - q[:host_samples]).max())
        # the device call serves S labellings, the host formula host_samples of them
        out['ratio_host_dense_over_community_per_labelling'] = (
            (out['host_dense_modularity_ms'] / host_samples) / (out['community_accumulate_ms'] / S))
    return out


def merged(path, cases):
    """the file's content with ``cases`` in it: a case measured before at the same shape and S is replaced, the
    others stay, so that runs with --samples / --shapes add up to one file"""
    key = lambda c: (c['S'], c['N'], c['T'], c['model'])
    kept = {}
    if os.path.exists(path):
        kept = {key(c): c for c in json.load(open(path))['cases']}
    kept.update({key(c): c for c in cases})
    return dict(what='dlsm_community_accumulate (K = %d, no blocks) against dlsm_post_cooccurrence on the same labels '
                     'and, at T=10 N=2000 and S=%d, the dense host modularity trace(S^T B S) / (2m) of '
                     'tests/community_ref.py; HIP events, host checks and copies included, median of %d; a case per '
                     'run of the script that measured it' % (K, HOST_SAMPLES, REPEATS),
                cases=[kept[k] for k in sorted(kept)])


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', default=','.join(str(s) for s in SAMPLES))
    ap.add_argument('--shapes', default='und,dir')
    ap.add_argument('--host-samples', type=int, default=HOST_SAMPLES)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'community_timing.json'))
    args = ap.parse_args()
    cases = []
    for S in [int(s) for s in args.samples.split(',')]:
        for shape in args.shapes.split(','):
            T, N, directed = SHAPES[shape]
            cases.append(measure(T, N, directed, S, args.host_samples if S == int(args.samples.split(',')[0]) else 0))
            print(json.dumps(cases[-1]), flush=True)
            json.dump(merged(args.out, cases), open(args.out, 'w'), indent=1)
    print(json.dumps(cases))
