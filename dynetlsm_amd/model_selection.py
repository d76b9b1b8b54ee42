"""Held-out dyads for link prediction: blank a share of every time slice's dyads as -1, fit with
``sample_missing=True`` and score ``missing_probas_`` on them (``metrics.heldout_scores``)."""
import numpy as np

__all__ = ['train_test_split']


def train_test_split(Y, test_size=0.1, random_state=None, is_directed=False):
    """Hold out ``round(test_size * n_dyads)`` dyads of every time slice, drawn without replacement
    (n_dyads = N (N - 1) / 2 pairs i < j of an undirected network, N (N - 1) arcs of a directed one).

    Returns ``(Y_train, index)``: a float64 copy of ``Y`` with the held-out dyads coded -1 (both
    entries of an undirected pair, so the copy stays symmetric; the diagonal is never touched) and
    the held-out dyads as (n, 3) int64 rows (t, i, j) in row-major order, i < j when undirected -
    the order of the estimators' ``missing_index_``."""
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
