"""``SparseNetwork``: a dynamic binary network as edge lists, one (n_t, 2) array of ordered pairs
(i, j) per time step.  What the estimators take in place of the dense (T, N, N) tensor when the
network is large and sparse: ``Chain.upload_network_edges`` turns the lists into the packed rows or
the case-control tables on the device, and nothing on the way into ``fit`` forms T x N x N values.

The container is model-agnostic: a directed estimator reads (i, j) as the tie i -> j, an undirected
one reads a pair in either orientation as the tie {i, j}.  Duplicates and any order within a step are
allowed.

Dyads that were not observed are a second set of lists, ``missing``, stored the same way (held-out
dyads of ``model_selection.train_test_split``, or the -1 entries of ``from_dense(Y,
missing_value=-1)``).  A directed estimator reads a missing pair (i, j) as the arc i -> j, an
undirected one reads either orientation as the dyad {i, j}; duplicates are allowed.  Whether a dyad
is listed both as a tie and as missing depends on that reading, so the device finds it out at upload
(``Chain.set_missing_edges``), not the constructor.  ``degrees`` and ``n_ties`` count ties only;
``to_dense`` writes -1 at the missing dyads.  ``DynamicNetworkLSM`` and ``DynamicNetworkHDPLPCM``
(host-driven loop) fit such a container, with ``sample_missing=True`` re-drawing the listed dyads
every iteration; ``DynamicNetworkLPCM`` and the case-control likelihood do not take missing lists.

``numpy.asarray(net)`` densifies (float64, T * N * N * 8 bytes) - that is what keeps the trace
passes (goodness of fit, information criteria, scores, ...) working on a sparse-fitted model, and it
is the only place that does.
"""
import numpy as np

__all__ = ['SparseNetwork']


def _pair_lists(lists, N, name):
    """``(offsets int64[T + 1], src int32[n], dst int32[n])`` of a sequence of T integer (n_t, 2) arrays,
    checked: integer dtype, shapes, indices in 0..N-1, no self loops"""
    if isinstance(lists, np.ndarray) and lists.ndim != 3:
        raise ValueError('%s must be a sequence of (n_t, 2) arrays, one per time step' % name)
    lists = list(lists)
    if not lists:
        raise ValueError('%s must hold at least one time step' % name)
    src, dst, counts = [], [], []
    for t, e in enumerate(lists):
        e = np.asarray(e)
        if e.size == 0:
            e = np.zeros((0, 2), dtype=np.int32)
        if e.dtype == bool or not np.issubdtype(e.dtype, np.integer):
            raise ValueError('%s[%d] must be an integer array, got dtype %s' % (name, t, e.dtype))
        if e.ndim != 2 or e.shape[1] != 2:
            raise ValueError('%s[%d] must have shape (n_t, 2), got %s' % (name, t, e.shape))
        if (e < 0).any() or (e >= N).any():
            raise ValueError('%s[%d] holds a node id outside 0..%d' % (name, t, N - 1))
        if (e[:, 0] == e[:, 1]).any():
            raise ValueError('%s[%d] holds a self loop: the diagonal is not a dyad' % (name, t))
        src.append(e[:, 0].astype(np.int32)); dst.append(e[:, 1].astype(np.int32))
        counts.append(e.shape[0])
    return (np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
            np.ascontiguousarray(np.concatenate(src), dtype=np.int32),
            np.ascontiguousarray(np.concatenate(dst), dtype=np.int32))


def _split_triples(tij, T, name):
    """(n, 3) integer rows (t, i, j) in any order -> the T (n_t, 2) arrays of their pairs"""
    tij = np.asarray(tij)
    if tij.size == 0:
        tij = np.zeros((0, 3), dtype=np.int64)
    if tij.dtype == bool or not np.issubdtype(tij.dtype, np.integer):
        raise ValueError('%s must be an integer array, got dtype %s' % (name, tij.dtype))
    if tij.ndim != 2 or tij.shape[1] != 3:
        raise ValueError('%s must have shape (n, 3), got %s' % (name, tij.shape,))
    if T < 1 or (tij[:, 0] < 0).any() or (tij[:, 0] >= T).any():
        raise ValueError('%s holds a time step outside 0..%d' % (name, T - 1))
    order = np.argsort(tij[:, 0], kind='stable')
    cuts = np.searchsorted(tij[order, 0], np.arange(T + 1))
    return [tij[order[cuts[t]:cuts[t + 1]], 1:] for t in range(T)]


class SparseNetwork(object):
    """``edges``: a sequence of T integer arrays of shape (n_t, 2) (an array may be empty);
    ``n_nodes``: N; ``missing``: None or T such arrays of the dyads that were not observed.  Checked
    here, before any device call: integer dtype, shapes, indices in 0..N-1, no self loops."""

    def __init__(self, edges, n_nodes, missing=None):
        if isinstance(n_nodes, bool) or int(n_nodes) != n_nodes or int(n_nodes) < 2:
            raise ValueError('n_nodes must be an integer >= 2, got %r' % (n_nodes,))
        N = int(n_nodes)
        if N >= 2 ** 31:
            raise ValueError('n_nodes=%d: node ids are 32-bit' % N)
        self._N = N
        self._offsets, self._src, self._dst = _pair_lists(edges, N, 'edges')
        if missing is None:
            self._moffsets = np.zeros(self._offsets.shape[0], dtype=np.int64)
            self._msrc = self._mdst = np.zeros(0, dtype=np.int32)
        else:
            self._moffsets, self._msrc, self._mdst = _pair_lists(missing, N, 'missing')
            if self._moffsets.shape[0] != self._offsets.shape[0]:
                raise ValueError('missing must hold one (m_t, 2) array per time step: %d for %d steps'
                                 % (self._moffsets.shape[0] - 1, self._offsets.shape[0] - 1))
        self._symmetric = False

    # -- construction ------------------------------------------------------------------------------
    @classmethod
    def from_triples(cls, tij, n_time_steps, n_nodes, missing=None):
        """(n, 3) integer rows (t, i, j), in any order; ``missing``: (m, 3) rows of missing dyads"""
        T = int(n_time_steps)
        return cls(_split_triples(tij, T, 'tij'), n_nodes,
                   None if missing is None else _split_triples(missing, T, 'missing'))

    @classmethod
    def from_dense(cls, Y, missing_value=None):
        """entries != 0 of ``Y`` (T, N, N) are ties; the diagonal is ignored.  ``missing_value=None``: -1
        (a missing dyad) raises ValueError; ``missing_value=-1``: those entries become the missing lists"""
        Y = np.asarray(Y)
        if Y.ndim != 3 or Y.shape[1] != Y.shape[2]:
            raise ValueError('Y must have shape (n_time_steps, n_nodes, n_nodes)')
        if missing_value is None and np.any(Y == -1):
            raise ValueError('Y holds -1 coded missing dyads: pass missing_value=-1 to list them as '
                             'missing (or impute them first)')
        edges, missing = [], []
        for t in range(Y.shape[0]):
            hole = np.zeros(Y[t].shape, dtype=bool) if missing_value is None else Y[t] == missing_value
            i, j = np.nonzero((Y[t] != 0) & ~hole)
            keep = i != j
            edges.append(np.stack([i[keep], j[keep]], axis=1))
            i, j = np.nonzero(hole)
            keep = i != j
            missing.append(np.stack([i[keep], j[keep]], axis=1))
        return cls(edges, Y.shape[1], None if missing_value is None else missing)

    @classmethod
    def from_scipy(cls, mats, missing_value=None):
        """a sequence of T ``scipy.sparse`` matrices (N, N); stored entries != 0 are ties, the
        diagonal is ignored; stored entries equal to ``missing_value`` (-1) are missing dyads - with the
        default a -1 raises ValueError"""
        mats = list(mats)
        if not mats:
            raise ValueError('mats must hold at least one time step')
        N = mats[0].shape[0]
        edges, missing = [], []
        for t, m in enumerate(mats):
            if m.shape != (N, N):
                raise ValueError('mats[%d] has shape %s, expected %s' % (t, m.shape, (N, N)))
            c = m.tocoo()
            if missing_value is None and np.any(c.data == -1):
                raise ValueError('mats[%d] holds -1 coded missing dyads' % t)
            hole = np.zeros(c.data.shape, dtype=bool) if missing_value is None else c.data == missing_value
            row, col = c.row.astype(np.int64), c.col.astype(np.int64)
            keep = (c.data != 0) & (row != col) & ~hole
            edges.append(np.stack([row[keep], col[keep]], axis=1))
            keep = hole & (row != col)
            missing.append(np.stack([row[keep], col[keep]], axis=1))
        return cls(edges, N, None if missing_value is None else missing)

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

    @property
    def has_missing(self):
        return bool(self._msrc.shape[0])

    @property
    def n_missing(self):
        """missing pairs per time step, as listed (duplicates count)"""
        return np.diff(self._moffsets)

    def missing_by_time(self):
        """``by_time`` of the missing lists - the layout ``dlsm_set_missing_edges`` takes"""
        return self._moffsets, self._msrc, self._mdst

    def _with(self, offsets, src, dst, moffsets, msrc, mdst):
        out = object.__new__(SparseNetwork)
        out.__dict__.update(self.__dict__)
        out._offsets, out._src, out._dst = offsets, src, dst
        out._moffsets, out._msrc, out._mdst = moffsets, msrc, mdst
        return out

    def without_missing(self):
        """the same ties (shared, not copied), no missing lists"""
        return self._with(self._offsets, self._src, self._dst, np.zeros_like(self._moffsets),
                          np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))

    def with_ties(self, index):
        """a container with the (n, 3) rows (t, i, j) added as ties (the first fill of the missing dyads)"""
        index = np.asarray(index, dtype=np.int64).reshape(-1, 3)
        T = self.n_time_steps
        add = _pair_lists(_split_triples(index, T, 'index'), self._N, 'index')
        src, dst, counts = [], [], []
        for t in range(T):
            for o, s, d in ((self._offsets, self._src, self._dst), add):
                src.append(s[o[t]:o[t + 1]]); dst.append(d[o[t]:o[t + 1]])
            counts.append(src[-1].shape[0] + src[-2].shape[0])
        return self._with(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
                          np.ascontiguousarray(np.concatenate(src), dtype=np.int32),
                          np.ascontiguousarray(np.concatenate(dst), dtype=np.int32),
                          self._moffsets, self._msrc, self._mdst)

    def _keys(self, t, symmetric, missing=False):
        """the distinct dyads of step t (ties, or the missing lists) as sorted int64 keys i * N + j"""
        o, s, d = ((self._moffsets, self._msrc, self._mdst) if missing else
                   (self._offsets, self._src, self._dst))
        lo, hi = o[t], o[t + 1]
        i, j = s[lo:hi].astype(np.int64), d[lo:hi].astype(np.int64)
        k = i * self._N + j
        if symmetric:
            k = np.concatenate([k, j * self._N + i])
        return np.unique(k)

    def lookup(self, index, symmetric=None):
        """the values at the (n, 3) rows (t, i, j): 1.0 a tie, -1.0 a listed missing dyad, else 0.0 (in
        either orientation when ``symmetric``; default: as the container is seen) - by sorted keys, no
        N x N array"""
        sym = self._symmetric if symmetric is None else bool(symmetric)
        index = np.asarray(index, dtype=np.int64).reshape(-1, 3)
        out = np.zeros(index.shape[0], dtype=np.float64)
        key = index[:, 1] * self._N + index[:, 2]
        for t in range(self.n_time_steps):
            at = np.nonzero(index[:, 0] == t)[0]
            if not at.shape[0]:
                continue
            for value, missing in ((1.0, False), (-1.0, True)):
                keys = self._keys(t, sym, missing)
                pos = np.minimum(np.searchsorted(keys, key[at]), max(keys.shape[0] - 1, 0))
                hit = keys[pos] == key[at] if keys.shape[0] else np.zeros(at.shape[0], dtype=bool)
                out[at[hit]] = value
        return out

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
        """the float64 (T, N, N) adjacency tensor; ``symmetric``: both orientations of every pair.  The
        listed missing dyads hold -1 (both entries when ``symmetric``)"""
        Y = np.zeros(self.shape, dtype=np.float64)
        for value, (o, s, d) in ((1.0, self.by_time()), (-1.0, self.missing_by_time())):
            for t in range(self.n_time_steps):
                lo, hi = o[t], o[t + 1]
                Y[t, s[lo:hi], d[lo:hi]] = value
                if symmetric:
                    Y[t, d[lo:hi], s[lo:hi]] = value
        return Y

    def __array__(self, dtype=None, copy=None):
        Y = self.to_dense(self._symmetric)
        return Y if dtype is None else Y.astype(dtype, copy=False)

    def __repr__(self):
        return 'SparseNetwork(T=%d, N=%d, pairs=%d%s%s)' % (
            self.n_time_steps, self._N, self._src.shape[0],
            ', missing=%d' % self._msrc.shape[0] if self.has_missing else '',
            ', symmetric' if self._symmetric else '')
