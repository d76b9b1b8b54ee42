"""The goodness-of-fit records (include/dynetlsm_hip.h: dlsm_gof_simulate, dlsm_gof_dynamic_simulate) from
edge lists and packed rows, without an N x N matrix: what tests/gof_stats.py and tests/gof_dynamic_ref.py
compute from dense networks, for the sizes at which those cannot run, and the networks that
tests/test_gpu_gof_shapes.py gives to the device.  tests/test_gof_rows_ref_cpu.py pins every function to
the two dense modules and holds every network to the conditions its test relies on.

A network over time is `edges`: a list of T integer arrays (m_t, 2) of rows (i, j).  A directed row is the
arc i -> j; an undirected row is the pair {i, j}, listed once in either order.  A row listed twice counts
once.  Packed rows are the engine's: (T, N, W) uint32, bit j % 32 of word j // 32 of row i = Y[t, i, j]."""
import functools

import numpy as np

GOF_HB = 2048           # histogram bins the kernels hold in LDS (csrc/kernels_gof.hpp)
GOF_CHUNK = 256         # row words per chunk of k_gof_stats and k_gof_step
COLS_PER_CHUNK = 32 * GOF_CHUNK
COLS_PER_SLOT = 32 * 64     # columns of one register slot of k_gof_geodesic


def row_words(N):
    return ((int(N) + 31) // 32 + 3) // 4 * 4


def lanes_per_row(W):
    """gof_lanes_per_row of csrc/capi_gof.hpp"""
    L = 1
    while L < W // 4 and L < 64:
        L <<= 1
    return L


def geodesic_slots(N):
    """(used slots, NW) of k_gof_geodesic at N nodes (gof_dynamic_launch)"""
    used = (row_words(N) + 63) // 64
    return used, next(nw for nw in (1, 2, 4, 8, 16) if used <= nw)


# ---- edge lists and packed rows -------------------------------------------------------------------------------
def dyads(N, e, directed):
    """the distinct dyads of one edge list as (i, j), sorted by i * N + j; undirected: i < j"""
    e = np.asarray(e, dtype=np.int64).reshape(-1, 2)
    i, j = e[:, 0], e[:, 1]
    assert ((i != j) & (i >= 0) & (j >= 0) & (i < N) & (j < N)).all()
    if not directed:
        i, j = np.minimum(i, j), np.maximum(i, j)
    k = np.unique(i * N + j)
    return k // N, k % N


def _keys(N, e, directed):
    i, j = dyads(N, e, directed)
    return i * N + j


def _arcs(N, e, directed):
    """every set entry (i, j) of the adjacency matrix: undirected lists mirrored"""
    i, j = dyads(N, e, directed)
    return (i, j) if directed else (np.concatenate([i, j]), np.concatenate([j, i]))


def _pack_arcs(N, i, j):
    W = row_words(N)
    out = np.zeros(N * W, dtype=np.uint32)
    if len(i):
        word = i * W + (j >> 5)
        order = np.argsort(word, kind='stable')
        word = word[order]
        val = np.left_shift(np.uint32(1), (j[order] & 31).astype(np.uint32))
        start = np.flatnonzero(np.r_[True, word[1:] != word[:-1]])
        out[word[start]] = np.bitwise_or.reduceat(val, start)
    return out.reshape(N, W)


def pack_edges(T, N, edges, directed, transposed=False):
    """(T, N, W) uint32 rows of the networks (engine.pack_network of the dense matrices); `transposed`: of
    their transposes (row j holds the arcs into j)"""
    assert len(edges) == T
    out = np.zeros((T, N, row_words(N)), dtype=np.uint32)
    for t in range(T):
        i, j = _arcs(N, edges[t], directed)
        out[t] = _pack_arcs(N, j, i) if transposed else _pack_arcs(N, i, j)
    return out


def dense(T, N, edges, directed):
    """(T, N, N) bool, for the sizes at which the dense references run"""
    Y = np.zeros((T, N, N), dtype=bool)
    for t in range(T):
        i, j = _arcs(N, edges[t], directed)
        Y[t, i, j] = True
    return Y


def edges_of_dense(Y, directed):
    Y = np.asarray(Y) != 0
    return [np.argwhere(A if directed else np.triu(A, 1)) for A in Y]


_POP16 = np.unpackbits(np.arange(65536, dtype='<u2').view(np.uint8).reshape(-1, 2), axis=1).sum(1).astype(np.uint8)


def popcount_rows(a):
    """(m, k) uint64 -> (m,) int64 set bits per row, by a table over the 16-bit pieces"""
    a = np.ascontiguousarray(a)
    return _POP16[a.view(np.uint16)].sum(-1, dtype=np.int64)


def _u64(rows):
    return np.ascontiguousarray(rows).view(np.uint64)


def and_popcounts(R, S, i, j):
    """popcount(R[i[k]] & S[j[k]]) for every k, over uint64 rows, a few MB of rows at a time"""
    out = np.zeros(len(i), dtype=np.int64)
    step = max(1, (1 << 22) // R.shape[1])
    for c in range(0, len(i), step):
        out[c:c + step] = popcount_rows(R[i[c:c + step]] & S[j[c:c + step]])
    return out


def _hist(values, N):
    values = np.asarray(values, dtype=np.int64)
    assert values.size == 0 or (values.min() >= 0 and values.max() < N)
    return np.bincount(values, minlength=N)[:N]


# ---- the records ----------------------------------------------------------------------------------------------
def stats_records(T, N, edges, directed):
    """(T, 2 + 3N) int64: edges, mutual, deg_out[N], deg_in[N], esp[N] (gof_stats.records)"""
    out = np.zeros((T, 2 + 3 * N), dtype=np.int64)
    rows = pack_edges(T, N, edges, directed)
    trows = pack_edges(T, N, edges, directed, transposed=True) if directed else rows
    for t in range(T):
        i, j = dyads(N, edges[t], directed)
        R, C = _u64(rows[t]), _u64(trows[t])
        out[t, 0] = len(i)
        out[t, 2:2 + N] = _hist(popcount_rows(R), N)
        if directed:
            out[t, 1] = int(np.isin(j * N + i, i * N + j)[i < j].sum())
            out[t, 2 + N:2 + 2 * N] = _hist(np.bincount(j, minlength=N), N)
        # partners m with i -> m -> j: row i against column j (undirected: row j)
        out[t, 2 + 2 * N:] = _hist(and_popcounts(R, C, i, j), N)
    return out


def overlap(T, N, edges, directed):
    """(T, T) int64 dyads present at both steps (gof_dynamic_ref.overlap), from the edge sets"""
    keys = [_keys(N, e, directed) for e in edges]
    return np.array([[len(np.intersect1d(a, b, assume_unique=True)) for b in keys] for a in keys],
                    dtype=np.int64).reshape(T, T)


def steps(T, N, edges, directed):
    """(T - 1, 2N) int64: persist_degree[N], formed_sp[N] per step (gof_dynamic_ref.steps)"""
    out = np.zeros((max(T - 1, 0), 2 * N), dtype=np.int64)
    rows = pack_edges(T, N, edges, directed)
    trows = pack_edges(T, N, edges, directed, transposed=True) if directed else rows
    for t in range(T - 1):
        A, B, At = _u64(rows[t]), _u64(rows[t + 1]), _u64(trows[t])
        out[t, :N] = _hist(popcount_rows(A & B), N)
        ka, kb = _keys(N, edges[t], directed), _keys(N, edges[t + 1], directed)
        formed = kb[~np.isin(kb, ka)]
        out[t, N:] = _hist(and_popcounts(A, At, formed // N, formed % N), N)
    return out


def _graph(N, e, directed):
    from scipy.sparse import csr_matrix
    i, j = _arcs(N, e, directed)
    return csr_matrix((np.ones(len(i)), (i, j)), shape=(N, N))


def geodesic_bfs(N, e, directed, chunk=1024):
    """(N,) int64 pairs by shortest-path length of one network, bin 0 the pairs without a path
    (gof_dynamic_ref.geodesic): a breadth-first search from every node, `chunk` sources at a time"""
    from scipy.sparse.csgraph import shortest_path
    G = _graph(N, e, directed)
    hist = np.zeros(N, dtype=np.int64)
    col = np.arange(N)
    for s0 in range(0, N, chunk):
        src = np.arange(s0, min(N, s0 + chunk))
        d = shortest_path(G, directed=True, unweighted=True, indices=src)
        target = col[None, :] != src[:, None] if directed else col[None, :] > src[:, None]
        d = np.where(np.isfinite(d), d, 0.0)[target]
        hist += _hist(np.rint(d), N)
    return hist


def geodesic_components(N, e, directed, sources):
    """the same for a disjoint union of vertex-transitive components (directed: strongly connected ones), of
    which `sources` names one node each, by one search per component: the n_c nodes of a component all see
    the distances h_c its source sees, so n_c * h_c ordered pairs, half as many pairs i < j; the pairs
    across components (the products of the component sizes) have no path and go to bin 0.  The node labels
    do not matter."""
    from scipy.sparse.csgraph import shortest_path
    d = shortest_path(_graph(N, e, directed), directed=True, unweighted=True, indices=np.asarray(sources))
    seen = np.isfinite(d)
    assert (seen.sum(0) == 1).all(), 'the sources do not name every component once'
    hist = np.zeros(N, dtype=np.int64)
    for c in range(len(sources)):
        h = _hist(np.rint(d[c][seen[c]]), N)
        h[0] = 0                                    # the source itself
        hist += int(seen[c].sum()) * h
    if not directed:
        assert (hist % 2 == 0).all()
        hist //= 2
    pairs = N * (N - 1) if directed else N * (N - 1) // 2
    sizes = seen.sum(1)
    across = (int(sizes.sum()) ** 2 - int((sizes ** 2).sum())) // (1 if directed else 2)
    assert pairs - int(hist.sum()) == across
    hist[0] = across
    return hist


def bfs_levels(N, e, directed, source):
    """(N,) int64 distance from `source` along the arcs, -1 where there is no path"""
    from scipy.sparse.csgraph import shortest_path
    d = shortest_path(_graph(N, e, directed), directed=True, unweighted=True, indices=[source])[0]
    return np.where(np.isfinite(d), d, -1.0).astype(np.int64)


# ---- small dense networks by the thousand ---------------------------------------------------------------------
def _batch_hist(values, mask, N):
    """histograms over all but the first axis: values (n, ...) int in [0, N), mask alike -> (n, N)"""
    n = values.shape[0]
    idx = np.arange(n).reshape((n,) + (1,) * (values.ndim - 1)) * N + values
    return np.bincount(idx[mask], minlength=n * N).reshape(n, N)


def _dyad_mask(N, directed):
    return ~np.eye(N, dtype=bool) if directed else np.triu(np.ones((N, N), dtype=bool), 1)


def batch_stats(Y, directed):
    """(..., N, N) bool -> (..., 2 + 3N) int64: gof_stats.records over the leading axes"""
    Y = np.asarray(Y) != 0
    lead, N = Y.shape[:-2], Y.shape[-1]
    Yn = Y.reshape((-1, N, N))
    A = Yn.astype(np.int64)
    dy, up = _dyad_mask(N, directed), _dyad_mask(N, False)
    out = np.zeros((Yn.shape[0], 2 + 3 * N), dtype=np.int64)
    out[:, 0] = (Yn & dy).sum((1, 2))
    out[:, 2:2 + N] = _batch_hist(A.sum(2), np.ones(A.shape[:2], dtype=bool), N)
    if directed:
        out[:, 1] = (Yn & Yn.swapaxes(1, 2) & up).sum((1, 2))
        out[:, 2 + N:2 + 2 * N] = _batch_hist(A.sum(1), np.ones(A.shape[:2], dtype=bool), N)
    out[:, 2 + 2 * N:] = _batch_hist(A @ A, Yn & dy, N)
    return out.reshape(lead + (2 + 3 * N,))


def batch_dynamic(Y, directed):
    """(S, T, N, N) bool -> overlap (S, T, T), steps (S, T - 1, 2N), geodesic (S, T, N) int64:
    gof_dynamic_ref.records over the samples"""
    Y = np.asarray(Y) != 0
    S, T, N, _ = Y.shape
    dy = _dyad_mask(N, directed)
    E = (Y & dy).reshape(S, T, N * N).astype(np.int64)
    ov = E @ E.swapaxes(1, 2)
    st = np.zeros((S, max(T - 1, 0), 2 * N), dtype=np.int64)
    if T > 1:
        A, B = Y[:, :-1].reshape(-1, N, N), Y[:, 1:].reshape(-1, N, N)
        Ai = A.astype(np.int64)
        st[..., :N] = _batch_hist((A & B).sum(2), np.ones(A.shape[:2], dtype=bool), N).reshape(S, T - 1, N)
        st[..., N:] = _batch_hist(Ai @ Ai, B & ~A & dy, N).reshape(S, T - 1, N)
    A = Y.reshape(-1, N, N)
    Ai = A.astype(np.int64)
    dist = np.zeros(A.shape, dtype=np.int64)
    visited = np.broadcast_to(np.eye(N, dtype=bool), A.shape).copy()
    frontier = visited.copy()
    for level in range(1, N):
        frontier = ((frontier.astype(np.int64) @ Ai) > 0) & ~visited
        dist[frontier] = level
        visited |= frontier
    geo = _batch_hist(dist, np.broadcast_to(dy, A.shape), N).reshape(S, T, N)
    return ov, st, geo


# ---- the draws, over the sample index -------------------------------------------------------------------------
def draw_params(seed, S, T, N, D, directed):
    """posterior samples as test_gpu_gof._params makes them"""
    rng = np.random.RandomState(seed)
    Xs = rng.randn(S, T, N, D) * (1.5 / np.sqrt(D))
    ic = np.stack([rng.uniform(-0.5, 1.5, S), rng.uniform(-0.5, 1.5, S)], axis=1)
    radii = rng.uniform(0.5, 2.0, (S, N)) if directed else None
    return Xs, ic, radii


def batch_uniforms(philox4x32, seed, first, S, T, N, directed):
    """(S, T, N, N) uniforms of the samples at RNG indices first .. first + S - 1: gof_stats.uniforms"""
    from gof_stats import u53
    i, j = np.triu_indices(N, 1)
    index = (first + np.arange(S, dtype=np.int64))[:, None]
    U = np.ones((S, T, N, N))
    for t in range(T):
        r0, r1, r2, r3 = philox4x32(seed, i[None, :], j[None, :], index, (t << 8) | 7)
        a = u53(r0, r1)
        U[:, t, i, j] = a
        U[:, t, j, i] = u53(r2, r3) if directed else a
    return U


def batch_probabilities(Xs, ic, radii, directed):
    """(S, T, N, N) edge probabilities: gof_stats.probabilities, the same operations in the same order"""
    d = np.sqrt(((Xs[:, :, :, None, :] - Xs[:, :, None, :, :]) ** 2).sum(-1))
    if directed:
        eta = (ic[:, 0, None, None, None] * (1 - d / radii[:, None, None, :]) +
               ic[:, 1, None, None, None] * (1 - d / radii[:, None, :, None]))
    else:
        eta = ic[:, 0, None, None, None] - d
    p = 1.0 / (1.0 + np.exp(-eta))
    idx = np.arange(Xs.shape[2])
    p[:, :, idx, idx] = 0.0
    return p


def host_draws(philox4x32, seed, first, Xs, ic, radii, directed):
    """the networks of the draws (S, T, N, N) bool, and where |u - p| >= 1e-12 leaves no doubt about them"""
    S, T, N, _ = Xs.shape
    U = batch_uniforms(philox4x32, seed, first, S, T, N, directed)
    P = batch_probabilities(Xs, ic, radii, directed)
    return U < P, np.abs(U - P) >= 1e-12


# ---- the networks of the device tests -------------------------------------------------------------------------
def random_dyads(rng, N, m, directed):
    """about m distinct random dyads (those drawn twice or on the diagonal are lost)"""
    i, j = rng.randint(0, N, m), rng.randint(0, N, m)
    i, j = dyads(N, np.stack([i, j], 1)[i != j], directed)
    return np.stack([i, j], 1)


def _cat(*parts):
    return np.concatenate([np.asarray(p, dtype=np.int64).reshape(-1, 2) for p in parts])


def _star(hub, others):
    others = np.asarray(others, dtype=np.int64)
    return np.stack([np.full(len(others), hub, dtype=np.int64), others], 1)


def _both_ways(e, directed):
    return _cat(e, e[:, ::-1]) if directed else e


def net_full_row(N, directed, seed=1):
    """density 0.1 at t = 0; at t = 1 seven in ten of those dyads stay and 0.03 of all form.  Node N // 3
    is tied to every other node at t = 1 (directed: by its out-arcs) and to every second one at t = 0, so
    its row has N - 1 neighbours and about N / 2 persisting and N / 2 formed ties."""
    rng = np.random.RandomState(seed)
    A0 = rng.rand(N, N) < 0.1
    A1 = (A0 & (rng.rand(N, N) < 0.7)) | (rng.rand(N, N) < 0.03)
    hub = N // 3
    Y = np.stack([A0, A1])
    if not directed:
        Y = np.triu(Y, 1) | np.triu(Y, 1).swapaxes(1, 2)
    Y[0, hub, ::2] = True
    Y[1, hub, :] = True
    if not directed:
        Y[0, ::2, hub] = True
        Y[1, :, hub] = True
    Y[:, np.arange(N), np.arange(N)] = False
    return dict(N=N, T=2, directed=directed, edges=edges_of_dense(Y, directed), hub=hub, claims=())


def net_clique(N, n_clique, directed, seed=2):
    """a clique on n_clique random nodes over a background of mean degree 3.  At t = 0 a random tenth of the
    clique's dyads is absent, at t = 1 one in 2000 (directed: arcs, each on its own, so that in- and
    out-degrees differ): degrees and shared partners of t = 1 lie just below n_clique, in a handful of bins.
    (The shared partners at t = 0, and with them formed_sp, lie near 0.81 n_clique; the persisting ties of
    a node near 0.9 n_clique.)"""
    rng = np.random.RandomState(seed)
    nodes = np.sort(rng.permutation(N)[:n_clique])
    a, b = np.triu_indices(n_clique, 1)
    full = np.stack([nodes[a], nodes[b]], 1)
    full = _both_ways(full, directed)
    back = random_dyads(rng, N, 3 * N // (1 if directed else 2), directed)
    keep = rng.rand(len(back))
    edges = [_cat(full[rng.rand(len(full)) >= 0.1], back[keep < 0.8]),
             _cat(full[rng.rand(len(full)) >= 0.0005], back[keep > 0.2])]
    claims = ('deg_out', 'esp') + (('deg_in',) if directed else ())
    return dict(N=N, T=2, directed=directed, edges=edges, claims=claims)


def net_hubs(N, directed, hubs, seed=3, n_common=2100, n_pair=5, n_late=20, must_have=()):
    """a background of mean degree 3, four fifths of it at both steps, and three hubs: each tied (directed:
    by arcs both ways) at both steps to the same n_common nodes, which include `must_have`; hubs 1 and 2 also
    to n_pair more; each hub from t = 1 on to n_late nodes of its own and to the other two hubs.  So the
    hubs keep >= n_common ties, their degrees are >= n_common + 2, and the hub dyads form with >= n_common
    shared partners and have >= n_common + 1 at t = 1 - two of them in one bin, the third n_pair higher."""
    rng = np.random.RandomState(seed)
    hubs = np.asarray(hubs, dtype=np.int64)
    free = np.setdiff1d(np.arange(N), np.concatenate([hubs, np.asarray(must_have, dtype=np.int64)]))
    free = rng.permutation(free)
    n_free = n_common - len(must_have)
    common = np.concatenate([np.asarray(must_have, dtype=np.int64), free[:n_free]])
    pair = free[n_free:n_free + n_pair]
    late = free[n_free + n_pair:n_free + n_pair + 3 * n_late].reshape(3, n_late)
    back = random_dyads(rng, N, 3 * N // (1 if directed else 2), directed)
    back = back[~np.isin(back, hubs).any(1)]            # the hubs' ties are the listed ones alone
    keep = rng.rand(len(back))
    both = _cat(*([_star(h, common) for h in hubs] + [_star(h, pair) for h in hubs[1:]]))
    new = _cat(*([_star(h, late[k]) for k, h in enumerate(hubs)] +
                 [[[hubs[0], hubs[1]], [hubs[0], hubs[2]], [hubs[1], hubs[2]]]]))
    edges = [_cat(_both_ways(both, directed), back[keep < 0.8]),
             _cat(_both_ways(both, directed), _both_ways(new, directed), back[keep > 0.2])]
    claims = ('deg_out', 'esp', 'persist_degree', 'formed_sp') + (('deg_in',) if directed else ())
    return dict(N=N, T=2, directed=directed, edges=edges, hubs=hubs, claims=claims)


GEO_JUMPS = (1, 67, 4099)


def _circulant(first, n, jumps):
    v = np.arange(n, dtype=np.int64)
    return _cat(*[np.stack([first + v, first + (v + s) % n], 1) for s in jumps if s % n])


def net_geodesic(N, directed, n_cycle=4400, seed=4):
    """under a fixed random relabelling of the nodes: at t = 0 the circulant on all N nodes with the jumps
    GEO_JUMPS (directed: the arcs v -> v + s only), at t = 1 a cycle on n_cycle nodes beside the circulant
    on the others.  `sources[t]` names one node of every component."""
    perm = np.random.RandomState(seed).permutation(N).astype(np.int64)
    e0 = _circulant(0, N, GEO_JUMPS)
    e1 = _cat(_circulant(0, n_cycle, (1,)), _circulant(n_cycle, N - n_cycle, GEO_JUMPS))
    return dict(N=N, T=2, directed=directed, edges=[perm[e0], perm[e1]], n_cycle=n_cycle,
                sources=[[int(perm[0])], [int(perm[0]), int(perm[n_cycle])]], claims=('geodesic',))


def net_sparse(N, T, directed, seed=5):
    rng = np.random.RandomState(seed)
    back = random_dyads(rng, N, 3 * N // (1 if directed else 2), directed)
    edges = [back[rng.rand(len(back)) < 0.8] for _ in range(T)]
    return dict(N=N, T=T, directed=directed, edges=edges, claims=())


# name -> (maker, arguments without `directed`); test_gpu_gof_shapes.py's docstring says what each is for
OBSERVED = {
    'row300': (net_full_row, dict(N=300)),
    'row700': (net_full_row, dict(N=700)),
    'clique2100': (net_clique, dict(N=2100, n_clique=2060)),
    'hubs4200': (net_hubs, dict(N=4200, hubs=(7, 2048, 4150))),
    'hubs8200': (net_hubs, dict(N=8200, hubs=(3, 4100, 8199), must_have=tuple(range(8192, 8199)))),
    'geo8200': (net_geodesic, dict(N=8200)),
    'geo16400': (net_geodesic, dict(N=16400)),
}


@functools.lru_cache(maxsize=None)
def observed_case(name, directed):
    """the network of a case; shared by the tests of one process, which leave it unchanged"""
    make, kw = OBSERVED[name]
    return make(directed=directed, **kw)


# drawn networks: name -> (T, N, D, S, models as `directed` flags, seed of the parameters)
DRAWN = {
    'one_workgroup': (3, 5, 1, 3000, (False, True), 41),
    'two_batches': (3, 4, 2, 22000, (False,), 42),
    'wide_draw': (1, 2100, 2, 1, (True,), 43),
}
DRAW_SEED, DRAW_FIRST = 0x60F5A9E5C0DE, 5


@functools.lru_cache(maxsize=None)
def drawn_case(name, directed):
    """(Xs, ic, radii, Y, sure) of a drawn case: the parameters, the host's draws and where they are sure"""
    from oracle import oracle as orc
    T, N, D, S, models, seed = DRAWN[name]
    assert directed in models
    Xs, ic, radii = draw_params(seed, S, T, N, D, directed)
    Y, sure = host_draws(orc.philox4x32, DRAW_SEED, DRAW_FIRST, Xs, ic, radii, directed)
    return Xs, ic, radii, Y, sure
