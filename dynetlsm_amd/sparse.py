"""``SparseNetwork``: a dynamic binary network as edge lists, one (n_t, 2) array of ordered pairs
(i, j) per time step.  What the estimators take in place of the dense (T, N, N) tensor when the
network is large and sparse: ``Chain.upload_network_edges`` turns the lists into the packed rows or
the case-control tables on the device, and nothing on the way into ``fit`` forms T x N x N values.

The container is model-agnostic: a directed estimator reads (i, j) as the tie i -> j, an undirected
one reads a pair in either orientation as the tie {i, j}.  Duplicates and any order within a step are
allowed.  Missing dyads have no sparse form yet: ``from_dense`` rejects -1 entries, and the
estimators reject ``sample_missing=True`` with a container.

``numpy.asarray(net)`` densifies (float64, T * N * N * 8 bytes) - that is what keeps the trace
passes (goodness of fit, information criteria, scores, ...) working on a sparse-fitted model, and it
is the only place that does.
"""
import numpy as np

__all__ = ['SparseNetwork']


class SparseNetwork(object):
    """``edges``: a sequence of T integer arrays of shape (n_t, 2) (an array may be empty);
    ``n_nodes``: N.  Checked here, before any device call: integer dtype, shapes, indices in
    0..N-1, no self loops."""

    def __init__(self, edges, n_nodes):
        if isinstance(n_nodes, bool) or int(n_nodes) != n_nodes or int(n_nodes) < 2:
            raise ValueError('n_nodes must be an integer >= 2, got %r' % (n_nodes,))
        N = int(n_nodes)
        if N >= 2 ** 31:
            raise ValueError('n_nodes=%d: node ids are 32-bit' % N)
        if isinstance(edges, np.ndarray) and edges.ndim != 3:
            raise ValueError('edges must be a sequence of (n_t, 2) arrays, one per time step')
        edges = list(edges)
        if not edges:
            raise ValueError('edges must hold at least one time step')
        src, dst, counts = [], [], []
        for t, e in enumerate(edges):
            e = np.asarray(e)
            if e.size == 0:
                e = np.zeros((0, 2), dtype=np.int32)
            if e.dtype == bool or not np.issubdtype(e.dtype, np.integer):
                raise ValueError('edges[%d] must be an integer array, got dtype %s' % (t, e.dtype))
            if e.ndim != 2 or e.shape[1] != 2:
                raise ValueError('edges[%d] must have shape (n_t, 2), got %s' % (t, e.shape))
            if (e < 0).any() or (e >= N).any():
                raise ValueError('edges[%d] holds a node id outside 0..%d' % (t, N - 1))
            if (e[:, 0] == e[:, 1]).any():
                raise ValueError('edges[%d] holds a self loop: the diagonal is not a dyad' % t)
            src.append(e[:, 0].astype(np.int32)); dst.append(e[:, 1].astype(np.int32))
            counts.append(e.shape[0])
        self._N = N
        self._offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self._src = np.ascontiguousarray(np.concatenate(src), dtype=np.int32)
        self._dst = np.ascontiguousarray(np.concatenate(dst), dtype=np.int32)
        self._symmetric = False

    # -- construction ------------------------------------------------------------------------------
    @classmethod
    def from_triples(cls, tij, n_time_steps, n_nodes):
        """(n, 3) integer rows (t, i, j), in any order"""
        tij = np.asarray(tij)
        if tij.size == 0:
            tij = np.zeros((0, 3), dtype=np.int64)
        if tij.dtype == bool or not np.issubdtype(tij.dtype, np.integer):
            raise ValueError('tij must be an integer array, got dtype %s' % tij.dtype)
        if tij.ndim != 2 or tij.shape[1] != 3:
            raise ValueError('tij must have shape (n, 3), got %s' % (tij.shape,))
        T = int(n_time_steps)
        if T < 1 or (tij[:, 0] < 0).any() or (tij[:, 0] >= T).any():
            raise ValueError('tij holds a time step outside 0..%d' % (T - 1))
        order = np.argsort(tij[:, 0], kind='stable')
        cuts = np.searchsorted(tij[order, 0], np.arange(T + 1))
        return cls([tij[order[cuts[t]:cuts[t + 1]], 1:] for t in range(T)], n_nodes)

    @classmethod
    def from_dense(cls, Y):
        """entries != 0 of ``Y`` (T, N, N) are ties; the diagonal is ignored; -1 (a missing dyad)
        raises ValueError"""
        Y = np.asarray(Y)
        if Y.ndim != 3 or Y.shape[1] != Y.shape[2]:
            raise ValueError('Y must have shape (n_time_steps, n_nodes, n_nodes)')
        if np.any(Y == -1):
            raise ValueError('Y holds -1 coded missing dyads: a SparseNetwork has no missing dyads '
                             '(fit the dense array, or impute them first)')
        edges = []
        for t in range(Y.shape[0]):
            i, j = np.nonzero(Y[t])
            keep = i != j
            edges.append(np.stack([i[keep], j[keep]], axis=1))
        return cls(edges, Y.shape[1])

    @classmethod
    def from_scipy(cls, mats):
        """a sequence of T ``scipy.sparse`` matrices (N, N); stored entries != 0 are ties, the
        diagonal is ignored"""
        mats = list(mats)
        if not mats:
            raise ValueError('mats must hold at least one time step')
        N = mats[0].shape[0]
        edges = []
        for t, m in enumerate(mats):
            if m.shape != (N, N):
                raise ValueError('mats[%d] has shape %s, expected %s' % (t, m.shape, (N, N)))
            c = m.tocoo()
            if np.any(c.data == -1):
                raise ValueError('mats[%d] holds -1 coded missing dyads' % t)
            keep = (c.data != 0) & (c.row != c.col)
            edges.append(np.stack([c.row[keep].astype(np.int64), c.col[keep].astype(np.int64)], axis=1))
        return cls(edges, N)

    # -- attributes --------------------------------------------------------------------------------
    @property
    def n_time_steps(self):
        return self._offsets.shape[0] - 1

    @property
    def n_nodes(self):
        return self._N

    @property
    def n_edges(self):
        """pairs per time step, as listed (duplicates count)"""
        return np.diff(self._offsets)

    @property
    def shape(self):
        return (self.n_time_steps, self._N, self._N)

    @property
    def symmetric(self):
        """whether ``__array__``, ``degrees`` and ``n_ties`` read a pair in either orientation as
        both (an undirected estimator stores its ``Y_fit_`` that way)"""
        return self._symmetric

    def as_seen(self, symmetric):
        """the same lists (shared, not copied) as an estimator sees them: ``symmetric=True`` for an
        undirected fit"""
        out = object.__new__(SparseNetwork)
        out.__dict__.update(self.__dict__)
        out._symmetric = bool(symmetric)
        return out

    def by_time(self):
        """(offsets int64[T + 1], src int32[n], dst int32[n]): the pairs of step t are
        src / dst[offsets[t]:offsets[t + 1]] - the layout ``dlsm_upload_network_edges`` takes"""
        return self._offsets, self._src, self._dst

    def _keys(self, t, symmetric):
        """the distinct dyads of step t as sorted int64 keys i * N + j"""
        lo, hi = self._offsets[t], self._offsets[t + 1]
        i, j = self._src[lo:hi].astype(np.int64), self._dst[lo:hi].astype(np.int64)
        k = i * self._N + j
        if symmetric:
            k = np.concatenate([k, j * self._N + i])
        return np.unique(k)

    def degrees(self, symmetric=None):
        """(T, N, 2) int64: column 0 the in-degree, column 1 the out-degree of the distinct directed
        pairs (of the symmetrised network when ``symmetric``; default: as the container is seen).
        Works on the lists alone: O(E log E), no N x N array."""
        sym = self._symmetric if symmetric is None else bool(symmetric)
        deg = np.zeros((self.n_time_steps, self._N, 2), dtype=np.int64)
        for t in range(self.n_time_steps):
            k = self._keys(t, sym)
            deg[t, :, 1] = np.bincount(k // self._N, minlength=self._N)
            deg[t, :, 0] = np.bincount(k % self._N, minlength=self._N)
        return deg

    def n_ties(self, symmetric=None):
        """number of distinct directed pairs over all steps (of the symmetrised network when
        ``symmetric``): ``to_dense(symmetric).sum()`` without the tensor"""
        sym = self._symmetric if symmetric is None else bool(symmetric)
        return int(sum(self._keys(t, sym).shape[0] for t in range(self.n_time_steps)))

    def to_dense(self, symmetric=False):
        """the float64 (T, N, N) adjacency tensor; ``symmetric``: both orientations of every pair"""
        Y = np.zeros(self.shape, dtype=np.float64)
        for t in range(self.n_time_steps):
            lo, hi = self._offsets[t], self._offsets[t + 1]
            Y[t, self._src[lo:hi], self._dst[lo:hi]] = 1.0
            if symmetric:
                Y[t, self._dst[lo:hi], self._src[lo:hi]] = 1.0
        return Y

    def __array__(self, dtype=None, copy=None):
        Y = self.to_dense(self._symmetric)
        return Y if dtype is None else Y.astype(dtype, copy=False)

    def __repr__(self):
        return 'SparseNetwork(T=%d, N=%d, pairs=%d%s)' % (self.n_time_steps, self._N, self._src.shape[0],
                                                          ', symmetric' if self._symmetric else '')
