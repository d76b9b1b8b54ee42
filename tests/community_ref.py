"""Numpy restatement of ``dlsm_community_accumulate`` (include/dynetlsm_hip.h) from dense arrays, written from
the definitions and not from the kernel: one-hot matrices and matrix products where the device walks bits.  Also the
reference's modularity in its own dense form, ``trace(S^T B S) / (2m)`` (network_statistics.py:43-61), against
which the decomposed formula of ``dynetlsm_amd.community`` is checked."""
import numpy as np


def effective(Y, excluded, directed):
    """(ties, excluded) as (T, N, N) booleans: no diagonal, an undirected dyad excluded by either orientation, no
    tie on an excluded dyad"""
    Y = np.asarray(Y) != 0
    T, N = Y.shape[:2]
    E = np.zeros_like(Y) if excluded is None else np.asarray(excluded).astype(bool).copy()
    if not directed:
        E = E | E.transpose(0, 2, 1)
    idx = np.arange(N)
    E[:, idx, idx] = False
    A = Y & ~E
    A[:, idx, idx] = False
    return A, E


def tables(Y, zs, K, directed, excluded=None, want_blocks=False):
    """clusters (S, T, K, 5), node_within (T, N), node_switch (T - 1, N), moved (S, T - 1), blocks (S, T, K, K, 2)
    or None - int64, as ``Chain.community_accumulate`` returns them"""
    zs = np.asarray(zs, dtype=np.int64)
    S, T, N = zs.shape
    A, E = effective(Y, excluded, directed)
    A, E = A.astype(np.int64), E.astype(np.int64)
    clusters = np.zeros((S, T, K, 5), dtype=np.int64)
    node_within = np.zeros((T, N), dtype=np.int64)
    blocks = np.zeros((S, T, K, K, 2), dtype=np.int64) if want_blocks else None
    for s in range(S):
        for t in range(T):
            H = np.eye(K, dtype=np.int64)[zs[s, t]]                # (N, K) one-hot
            ties, excl = H.T @ A[t] @ H, H.T @ E[t] @ H            # (K, K): from cluster a to cluster b
            clusters[s, t, :, 0] = H.sum(axis=0)
            clusters[s, t, :, 1] = np.diag(ties)
            clusters[s, t, :, 2] = H.T @ A[t].sum(axis=1)
            clusters[s, t, :, 3] = H.T @ A[t].sum(axis=0)
            clusters[s, t, :, 4] = np.diag(excl)
            node_within[t] += (A[t] * (zs[s, t][:, None] == zs[s, t][None, :])).sum(axis=1)
            if want_blocks:
                blocks[s, t, :, :, 0], blocks[s, t, :, :, 1] = ties, excl
    changed = zs[:, 1:] != zs[:, :-1]                              # (S, T - 1, N)
    return clusters, node_within, changed.sum(axis=0).astype(np.int64), changed.sum(axis=2).astype(np.int64), blocks


def dense_static_modularity(A, z, directed):
    """network_statistics.py:43-61 on one (N, N) 0/1 matrix: NaN without a tie"""
    A = np.asarray(A, dtype=np.float64)
    if directed:
        n_edges = A.sum()
        degree = 0.5 * (A.sum(axis=0) + A.sum(axis=1))
        B = 0.5 * (A + A.T)
    else:
        n_edges = A.sum() / 2
        degree = A.sum(axis=0)
        B = A
    if n_edges == 0:
        return float('nan')
    _, groups = np.unique(np.asarray(z), return_inverse=True)
    degree = degree.reshape(-1, 1)
    B = B - degree @ degree.T / (2 * n_edges)
    Smat = np.eye(groups.max() + 1)[groups]
    return float(np.trace(Smat.T @ B @ Smat) / (2 * n_edges))


def dense_modularity(Y, z, directed, excluded=None):
    """(per step (T,), their nanmean) of one labelling z (T, N): network_statistics.py:31-40, with the mean taken
    over the steps that have a tie"""
    A, _ = effective(Y, excluded, directed)
    per_t = np.array([dense_static_modularity(A[t], z[t], directed) for t in range(A.shape[0])])
    ok = ~np.isnan(per_t)
    return per_t, float(per_t[ok].mean()) if ok.any() else float('nan')


def decomposed_modularity(clusters, directed):
    """the formula of the issue on one (K, 5) table, in Python integers up to the last divisions"""
    rows = [[int(v) for v in row] for row in np.asarray(clusters).tolist()]
    within = sum(r[1] for r in rows)
    if directed:
        two_m = 2 * sum(r[2] for r in rows)
        null4 = sum((r[2] + r[3]) ** 2 for r in rows)              # 4 sum_a degree_a^2
        if two_m == 0:
            return float('nan')
        return (within - null4 / (4 * two_m)) / two_m
    two_m = sum(r[2] for r in rows)
    if two_m == 0:
        return float('nan')
    return (within - sum(r[2] ** 2 for r in rows) / two_m) / two_m
