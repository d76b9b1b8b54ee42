"""Held-out dyads for link prediction: blank a share of every time slice's dyads as -1, fit with
``sample_missing=True`` and score ``missing_probas_`` on them (``metrics.heldout_scores``)."""
import numpy as np

from .sparse import SparseNetwork

__all__ = ['train_test_split']


def _distinct_ranks(rng, n_dyads, n):
    """n distinct int64 ranks below n_dyads, sorted: the first n distinct values of a stream of uniform
    draws (every subset of that size is equally likely), drawn in batches; O(n) memory"""
    if 2 * n > n_dyads:         # the complement is the smaller set; n_dyads < 2 n elements are in budget
        out = np.ones(n_dyads, dtype=bool)
        out[_distinct_ranks(rng, n_dyads, n_dyads - n)] = False
        return np.nonzero(out)[0].astype(np.int64)
    seen = np.zeros(0, dtype=np.int64)          # distinct values, in the order of their first draw
    while seen.shape[0] < n:
        batch = rng.randint(0, n_dyads, size=int(1.1 * (n - seen.shape[0])) + 16, dtype=np.int64)
        both = np.concatenate([seen, batch])
        _, first = np.unique(both, return_index=True)
        seen = both[np.sort(first)]
    return np.sort(seen[:n])


def _unrank(rank, N, is_directed):
    """(i, j) of the row-major rank among the arcs i != j, or among the pairs i < j, in closed form"""
    if is_directed:
        i, c = rank // (N - 1), rank % (N - 1)
        return i, c + (c >= i)
    # row i starts at i (2 N - i - 1) / 2: a float estimate of the root, then exact integer steps
    i = np.floor(((2 * N - 1) - np.sqrt(np.maximum((2.0 * N - 1) ** 2 - 8.0 * rank, 0.0))) / 2).astype(np.int64)
    i = np.clip(i, 0, N - 2)
    start = lambda i: i * (2 * N - i - 1) // 2
    while True:
        high = start(i) > rank
        low = ~high & (i < N - 2) & (start(i + 1) <= rank)
        if not (high.any() or low.any()):
            break
        i = i - high + low
    return i, rank - start(i) + i + 1


def _split_sparse(net, test_size, random_state, is_directed):
    if not 0.0 < test_size < 1.0:
        raise ValueError('test_size must lie in (0, 1)')
    if net.has_missing:
        raise ValueError('the network already lists missing dyads: split the fully observed one')
    rng = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
    T, N, _ = net.shape
    n_dyads = N * (N - 1) if is_directed else N * (N - 1) // 2
    n_test = int(round(test_size * n_dyads))
    if n_test < 1:
        raise ValueError('test_size=%r holds out no dyad of a slice of %d' % (test_size, n_dyads))
    offsets, src, dst = net.by_time()
    edges, missing, rows = [], [], []
    for t in range(T):
        i, j = _unrank(_distinct_ranks(rng, n_dyads, n_test), N, is_directed)
        held = i * N + j                        # sorted: the ranks are row-major
        if not is_directed:
            held = np.sort(np.concatenate([held, j * N + i]))
        s, d = src[offsets[t]:offsets[t + 1]].astype(np.int64), dst[offsets[t]:offsets[t + 1]].astype(np.int64)
        key = s * N + d
        pos = np.minimum(np.searchsorted(held, key), held.shape[0] - 1)
        keep = held[pos] != key
        edges.append(np.stack([s[keep], d[keep]], axis=1))
        missing.append(np.stack([i, j], axis=1))
        rows.append(np.stack([np.full(n_test, t, dtype=np.int64), i, j], axis=1))
    return SparseNetwork(edges, N, missing), np.concatenate(rows).astype(np.int64)


def train_test_split(Y, test_size=0.1, random_state=None, is_directed=False):
    """Hold out ``round(test_size * n_dyads)`` dyads of every time slice, drawn without replacement
    (n_dyads = N (N - 1) / 2 pairs i < j of an undirected network, N (N - 1) arcs of a directed one).

    Returns ``(Y_train, index)``: a float64 copy of ``Y`` with the held-out dyads coded -1 (both
    entries of an undirected pair, so the copy stays symmetric; the diagonal is never touched) and
    the held-out dyads as (n, 3) int64 rows (t, i, j) in row-major order, i < j when undirected -
    the order of the estimators' ``missing_index_``.

    A ``SparseNetwork`` is split without any array of n_dyads or N x N elements (host memory and time
    O(n_test + ties)): the same number of dyads per slice, uniform over all subsets of that size, the
    same ``index``; ``net_train`` is a container with the held-out ties gone from the edge lists (both
    orientations of an undirected pair) and the held-out pairs as its missing lists.  For the same
    seed its draws are NOT those of the dense split."""
    if isinstance(Y, SparseNetwork):
        return _split_sparse(Y, test_size, random_state, is_directed)
    Y = np.asarray(Y)
    if Y.ndim != 3 or Y.shape[1] != Y.shape[2]:
        raise ValueError('Y must have shape (n_time_steps, n_nodes, n_nodes)')
    if not 0.0 < test_size < 1.0:
        raise ValueError('test_size must lie in (0, 1)')
    if isinstance(random_state, np.random.RandomState):
        rng = random_state
    else:
        rng = np.random.RandomState(random_state)
    T, N, _ = Y.shape
    if is_directed:
        ii, jj = np.nonzero(~np.eye(N, dtype=bool))
    else:
        ii, jj = np.triu_indices(N, 1)
    n_dyads = ii.shape[0]
    n_test = int(round(test_size * n_dyads))
    if n_test < 1:
        raise ValueError('test_size=%r holds out no dyad of a slice of %d' % (test_size, n_dyads))
    Y_train = np.array(Y, dtype=np.float64)
    rows = []
    for t in range(T):
        pick = np.sort(rng.choice(n_dyads, n_test, replace=False))
        i, j = ii[pick], jj[pick]
        Y_train[t, i, j] = -1.0
        if not is_directed:
            Y_train[t, j, i] = -1.0
        rows.append(np.stack([np.full(n_test, t, dtype=np.int64), i, j], axis=1))
    return Y_train, np.concatenate(rows).astype(np.int64)
